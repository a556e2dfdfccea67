"""An extended-precision reference of the hyperelastic element operators: K(u), r(u), the energy, diag K(u) and the mass matrix, evaluated in a
chosen floating-point type (np.longdouble: the 80-bit x87 format on x86-64, eps 1.1e-19) and vectorised over the elements of a mesh.

Written from the formulas alone, like test_independent_restatement.py (whose per-point algebra it restates in any dtype) and sharing no code
with oracle/: the basis of every kind is written out here, det and inverse of the 2 x 2 / 3 x 3 matrices by cofactors (np.linalg refuses
long double), the logarithm taken in the working type.  The inputs are the doubles the device reads -- vertices, u, rule points and weights,
Lame parameters -- and everything after them is computed in the working type, so that a 1e-12 bar against this reference measures the
device's error alone, also where cond(F) is large and a double reference would itself hold only ~cond(F) eps.

Conventions (those of the assemblers): reference domains [-1, 1]^d, simplices with vertices (-1, ..)(1, -1, ..)(-1, 1, ..)..; Hex27 and Tet10
take their geometry from the embedded Hex8 / Tet4 (the first 8 / 4 nodes); F = I + (grad u)^T; r_I = sum_q w |det J| P g_I; the block of the
node pair (I, J) of K is C(g_I, g_J) of the material's stress contraction; the dof of component i of node I is s I + i."""
import numpy as np

HEX_SIGNS = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]])
QUAD_SIGNS = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]])
HEX27_NODES = np.array([tuple(s) for s in HEX_SIGNS] + [
    (0, -1, -1), (-1, 0, -1), (-1, -1, 0), (1, 0, -1), (1, -1, 0), (0, 1, -1), (1, 1, 0), (-1, 1, 0), (0, -1, 1), (-1, 0, 1), (1, 0, 1), (0, 1, 1),
    (0, 0, -1), (0, -1, 0), (-1, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)])
TET10_EDGES = [(0, 1), (1, 2), (0, 2), (0, 3), (2, 3), (1, 3)]   # nodes 4 .. 9: the midpoints of these vertex pairs
KINDS = {"QUAD4": (4, 2), "TRI3": (3, 2), "HEX8": (8, 3), "TET4": (4, 3), "HEX27": (27, 3), "TET10": (10, 3)}
GEOMETRY = {"HEX27": "HEX8", "TET10": "TET4"}
MODELS = ("LINEAR_ELASTIC", "NEO_HOOKEAN", "STVK", "LAPLACE")   # LAPLACE: one component, P = grad u, psi = |grad u|^2 / 2, K_ab = g_a . g_b


def _simplex(xi, dt):
    """barycentric coordinates (d + 1,) and their constant gradients (d + 1, d) on the reference simplex"""
    d = len(xi)
    lam = np.empty(d + 1, dtype=dt)
    lam[0] = -(np.sum(xi) + (d - 2)) / 2
    lam[1:] = (1 + xi) / 2
    dl = np.zeros((d + 1, d), dtype=dt)
    dl[0, :] = dt(-0.5)
    dl[1:, :] = np.eye(d, dtype=dt) / 2
    return lam, dl


def shape(kind, xi, dt=np.longdouble):
    """(phi (n,), grad phi (n, d)) of the reference basis at xi, in dt"""
    xi = np.asarray(xi, dtype=np.float64).astype(dt)
    if kind in ("QUAD4", "HEX8"):
        sg = (QUAD_SIGNS if kind == "QUAD4" else HEX_SIGNS).astype(dt)
        d = sg.shape[1]
        f = (1 + sg * xi[None, :]) / 2                           # (n, d): the one-dimensional factors
        phi = np.prod(f, axis=1)
        g = np.empty_like(sg)
        for k in range(d):
            g[:, k] = sg[:, k] / 2 * np.prod(np.delete(f, k, axis=1), axis=1)
        return phi, g
    if kind in ("TRI3", "TET4"):
        return _simplex(xi, dt)
    if kind == "TET10":
        lam, dl = _simplex(xi, dt)
        phi = np.empty(10, dtype=dt)
        g = np.empty((10, 3), dtype=dt)
        phi[:4] = lam * (2 * lam - 1)
        g[:4] = (4 * lam - 1)[:, None] * dl
        for m, (i, j) in enumerate(TET10_EDGES):
            phi[4 + m] = 4 * lam[i] * lam[j]
            g[4 + m] = 4 * (lam[i] * dl[j] + lam[j] * dl[i])
        return phi, g
    if kind == "HEX27":
        nodes = HEX27_NODES.astype(dt)
        x = xi[None, :]
        v = np.where(nodes == 0, 1 - x * x, x * (x + nodes) / 2)   # (27, 3): quadratic Lagrange factors
        dv = np.where(nodes == 0, -2 * x, x + nodes / 2)
        phi = v[:, 0] * v[:, 1] * v[:, 2]
        g = np.stack([dv[:, 0] * v[:, 1] * v[:, 2], v[:, 0] * dv[:, 1] * v[:, 2], v[:, 0] * v[:, 1] * dv[:, 2]], axis=1)
        return phi, g
    raise ValueError(kind)


def det(A):
    """determinants of a stack (..., d, d), d = 2 or 3, by cofactors"""
    if A.shape[-1] == 2:
        return A[..., 0, 0] * A[..., 1, 1] - A[..., 0, 1] * A[..., 1, 0]
    return (A[..., 0, 0] * (A[..., 1, 1] * A[..., 2, 2] - A[..., 1, 2] * A[..., 2, 1])
            - A[..., 0, 1] * (A[..., 1, 0] * A[..., 2, 2] - A[..., 1, 2] * A[..., 2, 0])
            + A[..., 0, 2] * (A[..., 1, 0] * A[..., 2, 1] - A[..., 1, 1] * A[..., 2, 0]))


def inv(A):
    """inverses of a stack (..., d, d) by the adjugate"""
    D = det(A)
    B = np.empty_like(A)
    if A.shape[-1] == 2:
        B[..., 0, 0], B[..., 1, 1] = A[..., 1, 1], A[..., 0, 0]
        B[..., 0, 1], B[..., 1, 0] = -A[..., 0, 1], -A[..., 1, 0]
        return B / D[..., None, None]
    for i in range(3):
        for j in range(3):
            r = [k for k in range(3) if k != j]
            c = [k for k in range(3) if k != i]
            B[..., i, j] = (-1) ** (i + j) * (A[..., r[0], c[0]] * A[..., r[1], c[1]] - A[..., r[0], c[1]] * A[..., r[1], c[0]])
    return B / D[..., None, None]


def _stress(model, F, mu, lam, I):
    """P (E, d, d), psi (E,) and the magnitudes of their terms (the scales of their rounding) for the deformation gradients F (E, d, d)"""
    d = F.shape[-1]
    aF = np.abs(F)
    if model == "LAPLACE":                                           # (F: the gradient (E, 1, d); no parameters)
        half = F.dtype.type(1) / 2
        e = half * np.einsum("eij,eij->e", F, F)
        return F, e, aF, e
    if model == "NEO_HOOKEAN":
        J = det(F)
        lnJ = np.log(J)
        Fit = np.swapaxes(inv(F), 1, 2)
        P = mu * (F - Fit) + lam * lnJ[:, None, None] * Fit
        psi = mu / 2 * (np.einsum("eij,eij->e", F, F) - d) - mu * lnJ + lam / 2 * lnJ ** 2
        P_abs = mu * (aF + np.abs(Fit)) + lam * np.abs(lnJ)[:, None, None] * np.abs(Fit)
        psi_abs = mu / 2 * (np.einsum("eij,eij->e", F, F) + d) + mu * np.abs(lnJ) + lam / 2 * lnJ ** 2
        return P, psi, P_abs, psi_abs
    if model == "STVK":
        E = (np.einsum("eki,ekj->eij", F, F) - I) / 2
        trE = np.einsum("eii->e", E)
        S = 2 * mu * E + lam * trE[:, None, None] * I
        E_abs = (np.einsum("eki,ekj->eij", aF, aF) + I) / 2
        trE_abs = np.einsum("eii->e", E_abs)
        S_abs = 2 * mu * E_abs + lam * trE_abs[:, None, None] * I
        return (F @ S, mu * np.einsum("eij,eij->e", E, E) + lam / 2 * trE ** 2, aF @ S_abs,
                mu * np.einsum("eij,eij->e", E_abs, E_abs) + lam / 2 * trE_abs ** 2)
    if model == "LINEAR_ELASTIC":
        eps = (F + np.swapaxes(F, 1, 2)) / 2 - I
        tr = np.einsum("eii->e", eps)
        eps_abs = (aF + np.swapaxes(aF, 1, 2)) / 2 + I
        tr_abs = np.einsum("eii->e", eps_abs)
        return (2 * mu * eps + lam * tr[:, None, None] * I, mu * np.einsum("eij,eij->e", eps, eps) + lam / 2 * tr ** 2,
                2 * mu * eps_abs + lam * tr_abs[:, None, None] * I, mu * np.einsum("eij,eij->e", eps_abs, eps_abs) + lam / 2 * tr_abs ** 2)
    raise ValueError(model)


def _contraction(model, F, g, mu, lam, I):
    """the element blocks C(g_a, g_b)[i][j] of one point as an array (E, a, i, b, j)"""
    gg = np.einsum("eak,ebk->eab", g, g)
    if model == "LAPLACE":
        return gg[:, :, None, :, None]
    delta = gg[:, :, None, :, None] * I[None, None, :, None, :]
    if model == "LINEAR_ELASTIC":
        return (mu * delta + mu * np.einsum("ebi,eaj->eaibj", g, g) + lam * np.einsum("eai,ebj->eaibj", g, g))
    if model == "NEO_HOOKEAN":
        J = det(F)
        alpha = -mu + lam * np.log(J)
        A = np.einsum("eak,eki->eai", g, inv(F))                 # a = F^-T g
        return (lam * np.einsum("eai,ebj->eaibj", A, A) - alpha[:, None, None, None, None] * np.einsum("ebi,eaj->eaibj", A, A)
                + mu * delta)
    if model == "STVK":
        E = (np.einsum("eki,ekj->eij", F, F) - I) / 2
        S = 2 * mu * E + lam * np.einsum("eii->e", E)[:, None, None] * I
        bSa = np.einsum("ebk,ekl,eal->eab", g, S, g)
        Fg = np.einsum("eik,eak->eai", F, g)
        FFt = np.einsum("eik,ejk->eij", F, F)
        return (bSa[:, :, None, :, None] * I[None, None, :, None, :] + mu * np.einsum("ebi,eaj->eaibj", Fg, Fg)
                + mu * gg[:, :, None, :, None] * FFt[:, None, :, None, :] + lam * np.einsum("eai,ebj->eaibj", Fg, Fg))
    raise ValueError(model)


class Reference:
    """K(u), r(u), the energy and the mass of a whole mesh in the working type dt.

    kind: one of KINDS; model: one of MODELS; vertices (N, d), connectivity (E, n), weights (nq,), points (nq, d), u (s N,): the doubles the
    device reads; mu, lam: Lame parameters (LAPLACE: not read); rho: a density for the mass matrix, one value or one per element.
    Per element: ke (E, s n, s n), re (E, s n), psi (E,),
    me (E, s n, s n); the absolute scales of the residual (re_scale: sum over the points of |w det J P g|, re_term_scale: the same with P
    replaced by the sum of the magnitudes of its terms) and of the energy (psi_term: the magnitudes of the terms of psi); det_F_min.

    The entry-wise scale of K (term_scale and its assembled forms): per element
        T_e[(a, i), (b, j)] = sum_q w_q |det J_q| C(|g|_a, |g|_b)[i][j],   |g|_a = |J_q^-1|^T |ghat_a(xi_q)|,
    the absolute values taken entry by entry BEFORE the products, so that no cancellation is credited -- neither between the terms of C,
    nor between the points, nor inside J^-T ghat -- and C the contraction of the operator at u = 0 with every term positive (LAPLACE:
    |g|_a . |g|_b; LINEAR_ELASTIC and NEO_HOOKEAN: mu (|g|_a . |g|_b) delta_ij + mu |g|_b,i |g|_a,j + lam |g|_a,i |g|_b,j).  T_ij >= |K_ij|,
    and every entry of K, however small beside max |K|, is a sum of terms whose rounding is eps T_ij.  The scale of the mass matrix is sum_q w |det J|
    rho |phi_a| |phi_b| (me_scale): the linear bases are positive, so there it is the mass itself.  gamma: one factor per element folded
    into T_e (and me_scale) before assembling (coordinates far from the origin: see geometry_cases.element_gamma)."""

    def __init__(self, kind, model, vertices, connectivity, weights, points, u, mu, lam, rho=1.0, dt=np.longdouble):
        n, d = KINDS[kind]
        X = np.asarray(vertices, dtype=np.float64).astype(dt)
        conn = np.asarray(connectivity).astype(np.int64)
        assert conn.shape[1] == n and X.shape[1] == d
        E = len(conn)
        s = 1 if model == "LAPLACE" else d
        U = np.asarray(u).reshape(-1, s).astype(dt)                 # (u may come in dt itself: the steps of a difference quotient)
        mu, lam = dt(float(mu)), dt(float(lam))
        rho = np.broadcast_to(np.asarray(rho, dtype=np.float64).astype(dt).reshape(-1), (E,)) if np.size(rho) in (1, E) else None
        assert rho is not None, "rho: one value or one per element"
        I = np.eye(d, dtype=dt)
        gkind = GEOMETRY.get(kind, kind)
        ng = KINDS[gkind][0]
        Xe = X[conn[:, :ng]]                                          # (E, ng, d)
        Ue = U[conn]                                                  # (E, n, s)
        ke = np.zeros((E, n, s, n, s), dtype=dt)
        me = np.zeros((E, n, n), dtype=dt)
        me_abs = np.zeros((E, n, n), dtype=dt)
        re = np.zeros((E, n, s), dtype=dt)
        re_scale = np.zeros((E, n, s), dtype=dt)
        re_term = np.zeros((E, n, s), dtype=dt)
        psi = np.zeros(E, dtype=dt)
        psi_term = np.zeros(E, dtype=dt)
        det_F_min = np.inf
        for wq, xi in zip(np.asarray(weights, dtype=np.float64), np.asarray(points, dtype=np.float64).reshape(-1, d)):
            phi, G = shape(kind, xi, dt)
            _, Gg = shape(gkind, xi, dt)
            Jm = np.einsum("eni,nj->eij", Xe, Gg)                     # J[i][j] = sum_n x_n[i] d phi_n / d xi_j
            detJ = det(Jm)
            g = np.einsum("nk,ekj->enj", G, inv(Jm))                  # physical gradients J^-T ghat, (E, n, d)
            scale = dt(wq) * np.abs(detJ)
            F = np.einsum("enc,enj->ecj", Ue, g)                      # (grad u)^T
            if model != "LAPLACE":
                F = I + F                                             # F = I + (grad u)^T
                det_F_min = min(det_F_min, float(det(F).min()))
            P, ps, P_abs, ps_abs = _stress(model, F, mu, lam, I)
            psi += scale * ps
            psi_term += scale * ps_abs
            re += scale[:, None, None] * np.einsum("eij,eaj->eai", P, g)
            re_scale += scale[:, None, None] * np.abs(np.einsum("eij,eaj->eaij", P, g)).sum(axis=3)
            re_term += scale[:, None, None] * np.einsum("eij,eaj->eai", P_abs, np.abs(g))
            ke += scale[:, None, None, None, None] * _contraction(model, F, g, mu, lam, I)
            me += (rho * scale)[:, None, None] * np.outer(phi, phi)[None]
            me_abs += (np.abs(rho) * scale)[:, None, None] * np.outer(np.abs(phi), np.abs(phi))[None]
        self.kind, self.model, self.dt, self.s, self.n = kind, model, dt, s, n
        self._geometry = (gkind, Xe, np.asarray(weights, dtype=np.float64), np.asarray(points, dtype=np.float64).reshape(-1, d), mu, lam, I)
        self._scales = {}
        self.conn, self.num_nodes = conn, len(X)
        self.ke = ke.reshape(E, n * s, n * s)
        self.me = np.einsum("eab,ij->eaibj", me, np.eye(s, dtype=dt)).reshape(E, n * s, n * s)
        self.me_scale = np.einsum("eab,ij->eaibj", me_abs, np.eye(s, dtype=dt)).reshape(E, n * s, n * s)   # (the terms of M taken positive)
        self.re, self.re_scale, self.re_term_scale = re.reshape(E, -1), re_scale.reshape(E, -1), re_term.reshape(E, -1)
        self.psi, self.psi_term = psi, psi_term
        self.det_F_min = det_F_min
        self.dofs = (s * conn[:, :, None] + np.arange(s)[None, None, :]).reshape(E, -1)   # (E, s n)
        ndof = s * self.num_nodes
        rows = np.repeat(self.dofs, n * s, axis=1).reshape(-1)
        cols = np.tile(self.dofs, (1, n * s)).reshape(-1)
        self._keys = rows * ndof + cols
        self.pattern_keys = np.unique(self._keys)                    # sorted: row-major order of a CSR pattern with sorted columns
        self._slot = np.searchsorted(self.pattern_keys, self._keys)
        self.ndof = ndof

    # ---- global quantities (sums over the elements in the working type)
    def _on_pattern(self, elem):
        v = np.zeros(len(self.pattern_keys), dtype=self.dt)
        np.add.at(v, self._slot, elem.reshape(-1))
        return v

    def _vector(self, elem):
        v = np.zeros(self.ndof, dtype=self.dt)
        np.add.at(v, self.dofs.reshape(-1), elem.reshape(-1))
        return v

    def pattern(self):
        """(row_offsets, col_indices) of the pattern: every dof pair of every element"""
        rows, cols = np.divmod(self.pattern_keys, self.ndof)
        ro = np.zeros(self.ndof + 1, dtype=np.int64)
        np.add.at(ro, rows + 1, 1)
        return np.cumsum(ro), cols

    def csr_values(self, row_offsets, col_indices, which="K"):
        """K (or the mass "M") on a CSR pattern, which must equal this one"""
        ro, ci = np.asarray(row_offsets).astype(np.int64), np.asarray(col_indices).astype(np.int64)
        rows = np.repeat(np.arange(len(ro) - 1), np.diff(ro))
        assert np.array_equal(rows * self.ndof + ci, self.pattern_keys), "the pattern differs"
        return self._on_pattern(self.ke if which == "K" else self.me)

    def residual(self):
        return self._vector(self.re)

    def residual_scale(self, terms=False):
        """per dof: sum over elements and points of |w det J P g| (terms=True: of the magnitudes of the terms of P)"""
        return self._vector(self.re_term_scale if terms else self.re_scale)

    def energy(self):
        return np.sum(self.psi)

    def energy_scale(self, terms=False):
        """sum_e |psi_e| (terms=True: the sum of the magnitudes of the terms of psi)"""
        return np.sum(self.psi_term) if terms else np.sum(np.abs(self.psi))

    def diagonal(self, which="K"):
        m = self.ke if which == "K" else self.me
        return self._vector(np.diagonal(m, axis1=1, axis2=2))

    def apply(self, x, alpha=0.0, beta=1.0):
        """(alpha M + beta K) x, and the bound || (|alpha| |M| + |beta| |K|) |x| ||_inf with the assembled matrices"""
        x = np.asarray(x).astype(self.dt)
        ae = self.dt(float(alpha)) * self.me + self.dt(float(beta)) * self.ke if alpha else self.dt(float(beta)) * self.ke
        y = self._vector(np.einsum("eab,eb->ea", ae, x[self.dofs]))
        return y, float(np.max(self.abs_apply(x, alpha, beta)))

    def abs_apply(self, x, alpha=0.0, beta=1.0):
        """(|alpha| |M| + |beta| |K|) |x| with the assembled matrices, row by row: the scale of the rounding of every row of apply"""
        x = np.asarray(x).astype(self.dt)
        rows, cols = np.divmod(self.pattern_keys, self.ndof)
        if not hasattr(self, "_abs_k"):                              # (the assembled |K| and |M| on the pattern: formed once)
            self._abs_k, self._abs_m = np.abs(self._on_pattern(self.ke)), np.abs(self._on_pattern(self.me))
        k = abs(self.dt(float(beta))) * self._abs_k
        if alpha:
            k = k + abs(self.dt(float(alpha))) * self._abs_m
        b = np.zeros(self.ndof, dtype=self.dt)
        np.add.at(b, rows, k * np.abs(x[cols]))
        return b

    # ---- the entry-wise scale of K and M (see the class's docstring)
    def term_scale(self):
        """T_e (E, s n, s n) in the working type"""
        if "T" not in self._scales:
            assert self.model in ("LAPLACE", "LINEAR_ELASTIC", "NEO_HOOKEAN"), "term_scale: the operators that are linear, or taken at u = 0"
            gkind, Xe, weights, points, mu, lam, I = self._geometry
            E, n, s = len(Xe), self.n, self.s
            te = np.zeros((E, n, s, n, s), dtype=self.dt)
            model = "LAPLACE" if self.model == "LAPLACE" else "LINEAR_ELASTIC"
            for wq, xi in zip(weights, points):
                _, G = shape(self.kind, xi, self.dt)
                _, Gg = shape(gkind, xi, self.dt)
                Jm = np.einsum("eni,nj->eij", Xe, Gg)
                ag = np.einsum("nk,ekj->enj", np.abs(G), np.abs(inv(Jm)))            # |g|_a = |J^-1|^T |ghat_a|
                te += (self.dt(abs(wq)) * np.abs(det(Jm)))[:, None, None, None, None] * _contraction(model, None, ag, abs(mu), abs(lam), I)
            self._scales["T"] = te.reshape(E, n * s, n * s)
        return self._scales["T"]

    def _scaled(self, which, gamma):
        elem = self.term_scale() if which == "K" else self.me_scale
        if gamma is None:
            return elem
        return np.asarray(gamma, dtype=np.float64).astype(self.dt).reshape(-1, 1, 1) * elem

    def csr_term_scale(self, row_offsets, col_indices, which="K", gamma=None):
        """T (which="M": |M|) assembled on a CSR pattern, which must equal this one"""
        ro, ci = np.asarray(row_offsets).astype(np.int64), np.asarray(col_indices).astype(np.int64)
        rows = np.repeat(np.arange(len(ro) - 1), np.diff(ro))
        assert np.array_equal(rows * self.ndof + ci, self.pattern_keys), "the pattern differs"
        return self._on_pattern(self._scaled(which, gamma))

    def diagonal_term_scale(self, which="K", gamma=None):
        return self._vector(np.diagonal(self._scaled(which, gamma), axis1=1, axis2=2))

    def abs_apply_terms(self, x, alpha=0.0, beta=1.0, gamma=None):
        """(|alpha| |M| + |beta| T) |x| row by row, summed element by element: the scale of the rounding of every row of apply"""
        ax = np.abs(np.asarray(x).astype(self.dt))[self.dofs]
        ae = abs(self.dt(float(beta))) * self._scaled("K", gamma) if beta else 0
        if alpha:
            ae = ae + abs(self.dt(float(alpha))) * self._scaled("M", gamma)
        return self._vector(np.einsum("eab,eb->ea", ae, ax))
