"""NumPy statement of the lagged, smoothed Coulomb friction of fh_set_friction (include/fenris_hip.h), for tests/test_friction.py, on top
of contact_reference.py and dynamics_reference.py (both imported unchanged).

Obstacle o has a coefficient mu_o; eps is the slip length and ubar the lag displacement.  With xbar_i = X_i + ubar_i (constants of u):
    nbar = grad phi_o(xbar_i),  P = I - nbar nbar^T,  lam = k_o w_i max(0, -phi_o(xbar_i))
and with the slip s = P d_i (d_i = u_i - ubar_i), y = |s|:
    D   = sum_o sum_i mu_o lam f0(y)                    f0 = -y^3 / (3 eps^2) + y^2 / eps + eps / 3  (y < eps),  y  otherwise
    q_i = sum_o mu_o lam c1 s                           c1 = 2 / eps - y / eps^2  (y < eps),  1 / y  otherwise
    H_i = sum_o mu_o lam (c1 P - c2 s s^T)              c2 = 1 / (eps^2 y)  (0 < y < eps),  0  (y == 0),  1 / y^3  otherwise
A node out of contact at xbar, or at the centre of a ball or cavity there, gets nothing from that obstacle.  Every function takes the slip
vector d beside the lag displacement, so that central differences (lag state: the current u; d = dt v_h) use the same statement; `dtype`
np.longdouble runs the same arithmetic in extended precision.  LongDoubleElastic (below) is the whole problem in np.longdouble -- the
LinearElastic residual, the mass, the contact force -- and on it the integrators and Newton run in np.longdouble throughout: the tests
measure the rounding of the float64 run of the reference against that run.

The three integrators repeat dynamics_reference's with the lag rules of the header: central differences evaluate the term at the current
position with the slip of the half-step velocity (a_0: v_0) and eps = eps_v dt; Newmark and backward Euler set ubar = u_n and eps = eps_v dt
at the start of step n, and Newmark's a_0 is formed with ubar = u_0 (no friction force)."""
import numpy as np
import scipy.sparse as sp

import contact_reference as cr
import dynamics_reference as dr


def _eval(ob, x, dtype):
    """(phi, n or None) of one obstacle at x, in `dtype`"""
    kind, p, q, _ = ob
    d = len(x)
    p = np.asarray(p, dtype=dtype)[:d]
    if kind == "half_space":
        n = np.asarray(q, dtype=dtype)[:d]
        n = n / np.sqrt(n @ n)
        return (x - p) @ n, n
    y = x - p
    r = np.sqrt(y @ y)
    sign = dtype(1.0) if kind == "ball" else dtype(-1.0)
    return sign * (r - dtype(q)), (None if r == 0 else sign * y / r)


def _coefficients(y, eps):
    """(f0, c1, c2) at the slip y"""
    if y < eps:
        return -y ** 3 / (3 * eps * eps) + y * y / eps + eps / 3, 2 / eps - y / (eps * eps), (1 / (eps * eps * y) if y > 0 else y * 0)
    return y, 1 / y, 1 / y ** 3


def _visit(obstacles, mu, X, ubar, d, w, dtype):
    """yields (node, mu lam, nbar, s, y) for every active pair"""
    X = np.asarray(X)
    xbar = X.astype(dtype) + np.asarray(ubar, dtype=dtype).reshape(X.shape)
    d = np.asarray(d, dtype=dtype).reshape(X.shape)
    w = np.ones(len(X), dtype=dtype) if w is None else np.asarray(w, dtype=dtype)
    for ob, m in zip(obstacles, mu):
        if not m > 0.0:
            continue
        for i in range(len(X)):
            phi, n = _eval(ob, xbar[i], dtype)
            if not phi < 0 or n is None:
                continue
            s = d[i] - n * (n @ d[i])
            yield i, dtype(m) * (dtype(ob[3]) * w[i] * -phi), n, s, np.sqrt(s @ s)


def potential(obstacles, mu, X, ubar, d, eps, w=None, dtype=np.float64):
    eps = dtype(eps)
    return sum((ml * _coefficients(y, eps)[0] for _, ml, _, _, y in _visit(obstacles, mu, X, ubar, d, w, dtype)), dtype(0.0))


def force(obstacles, mu, X, ubar, d, eps, w=None, dtype=np.float64):
    eps = dtype(eps)
    q = np.zeros(np.shape(X), dtype=dtype)
    for i, ml, _, s, y in _visit(obstacles, mu, X, ubar, d, w, dtype):
        q[i] += ml * _coefficients(y, eps)[1] * s
    return q.reshape(-1)


def blocks(obstacles, mu, X, ubar, d, eps, w=None, dtype=np.float64):
    """H[i] (dim x dim) per node"""
    eps = dtype(eps)
    N, dim = np.shape(X)
    H = np.zeros((N, dim, dim), dtype=dtype)
    for i, ml, n, s, y in _visit(obstacles, mu, X, ubar, d, w, dtype):
        _, c1, c2 = _coefficients(y, eps)
        H[i] += ml * (c1 * (np.eye(dim, dtype=dtype) - np.outer(n, n)) - c2 * np.outer(s, s))
    return H


def tangent(obstacles, mu, X, ubar, d, eps, w=None):
    return sp.block_diag(list(blocks(obstacles, mu, X, ubar, d, eps, w)), format="csr")


class FrictionProblem:
    """wraps a contact problem (cr.ContactMixin on dr.Problem): residual, energy and tangent with the friction term at the wrapper's lag
    state (ubar, eps); everything else is the wrapped problem's"""

    def __init__(self, prob, mu, eps=None, ubar=None, dtype=np.float64):
        self.prob, self.mu, self.eps, self.dtype = prob, list(mu), eps, dtype
        self.out = np.longdouble if getattr(prob, "dtype", None) is np.longdouble else np.float64    # (a LongDoubleElastic: nothing is rounded to double)
        if self.out is np.longdouble:
            self.dtype = np.longdouble
        self.ubar = np.zeros(prob.n, dtype=self.out) if ubar is None else np.array(ubar, dtype=self.out)

    def __getattr__(self, name):
        return getattr(self.prob, name)

    def _args(self, u):
        return self.prob.obstacles, self.mu, self.prob.vertices, self.ubar, np.asarray(u) - self.ubar, self.eps, self.prob.node_weights

    def friction_force(self, u):
        return force(*self._args(u), dtype=self.dtype).astype(self.out)

    def friction_potential(self, u):
        return float(potential(*self._args(u), dtype=self.dtype))

    def slip(self, u):
        """per node the largest |s| over the active pairs (0: none)"""
        out = np.zeros(self.prob.N)
        ob, mu, X, ubar, d, _, w = self._args(u)
        for i, _, _, _, y in _visit(ob, mu, X, ubar, d, w, self.dtype):
            out[i] = max(out[i], float(y))
        return out

    def residual(self, u):
        return self.prob.residual(u) + self.friction_force(u)

    def energy(self, u):
        return self.prob.energy(u)   # (the records keep the stored energy: the dissipated work is not recorded)

    def tangent(self, u):
        return (self.prob.tangent(u) + tangent(*self._args(np.asarray(u, dtype=np.float64)))).tocsr()

    def explicit_force(self, u, v, dt):
        """central differences: the lag state is u, the slip dt v"""
        p = self.prob
        return force(p.obstacles, self.mu, p.vertices, u, dt * np.asarray(v), self.eps, p.node_weights, dtype=self.dtype).astype(self.out)


def central_difference(fp, u0, v0, dt, steps, eps_v):
    """(u, v, a, trajectory of u) after `steps` steps; fp: a FrictionProblem"""
    prob = fp.prob
    fp.eps = eps_v * dt
    fr = prob.free
    m = prob.lumped()
    u = np.array(u0, dtype=fp.out)
    v = np.where(fr, v0, 0.0).astype(fp.out)
    a = np.zeros(prob.n, dtype=fp.out)
    a[fr] = (prob.lf(0) * prob.f - prob.residual(u) - fp.explicit_force(u, v, dt))[fr] / m[fr]
    traj = [u.copy()]
    for j in range(steps):
        vh = v + 0.5 * dt * a
        u = np.where(fr, u + dt * vh, u)
        a = np.zeros(prob.n, dtype=fp.out)
        a[fr] = (prob.lf(j + 1) * prob.f - prob.residual(u) - fp.explicit_force(u, vh, dt))[fr] / m[fr]
        v = np.where(fr, vh + 0.5 * dt * a, 0.0)
        traj.append(u.copy())
    return u, v, a, np.array(traj)


def implicit(fp, scheme, u0, v0, dt, steps, eps_v, beta=0.25, gamma=0.5, tol=1e-8, backtracking=True, max_it=60):
    """Newmark(beta, gamma) ("newmark") or backward Euler ("euler") with ubar = u_n, eps = eps_v dt per step: (status, u, v, a, trajectory)"""
    prob = fp.prob
    fp.eps = eps_v * dt
    fr = prob.free
    M = prob.mass()
    euler = scheme == "euler"
    nb = 1.0 if euler else beta
    u = np.array(u0, dtype=fp.out)
    v = np.where(fr, v0, 0.0).astype(fp.out)
    a = np.zeros(prob.n, dtype=fp.out)
    M64 = M if sp.issparse(M) else sp.csr_matrix(np.asarray(M, dtype=np.float64))
    if not euler:
        a = prob.solve_free(M, prob.lf(0) * prob.f - prob.residual(u))   # (ubar = u_0: no friction force)
    traj = [u.copy()]
    for j in range(steps):
        fp.ubar = u.copy()
        load = prob.lf(j + 1) * prob.f
        u_ref = np.where(fr, u + dt * v + (0.0 if euler else dt * dt * (0.5 - beta)) * a, u)

        def F(x):
            out = M @ (x - u_ref) + nb * dt * dt * (fp.residual(x) - load)
            out[~fr] = 0.0
            return out

        def J(x):
            return (M64 + nb * dt * dt * fp.tangent(x)).tocsr()

        if fp.out is np.longdouble:
            status, un, _ = newton_ld(prob, F, J, u_ref.copy(), tol, max_it)
        else:
            status, un, _ = dr.newton(prob, F, J, u_ref.copy(), tol, backtracking, max_it)
        if status != "ok":
            return status, u, v, a, np.array(traj)
        if euler:
            vn = np.where(fr, (un - u) / dt, 0.0)
            a = np.where(fr, (vn - v) / dt, 0.0)
            v = vn
        else:
            an = np.where(fr, (un - u_ref) / (beta * dt * dt), 0.0)
            v = np.where(fr, v + dt * ((1.0 - gamma) * a + gamma * an), 0.0)
            a = an
        u = un
        traj.append(u.copy())
    return "ok", u, v, a, np.array(traj)


def newton(fp, u0, f, tol, backtracking=True, max_it=60):
    """the static solve r + g + q = f at the wrapper's lag state: (status, u, iterations)"""
    fr = fp.prob.free

    def F(x):
        out = fp.residual(x) - f
        out[~fr] = 0.0
        return out

    if fp.out is np.longdouble:
        return newton_ld(fp.prob, F, fp.tangent, u0, tol, max_it)
    return dr.newton(fp.prob, F, fp.tangent, np.array(u0, dtype=np.float64), tol, backtracking, max_it)


# ---- the reference in extended precision: linear elasticity on Hex8 / Tet4, the contact force, the friction term and the integrators all in
# np.longdouble, so that the float64 run of the reference has something to be measured against
LD = np.longdouble


def _shape_gradients(kind, xi):
    """dN/dxi of the element at the reference point xi: (nodes, 3)"""
    xi = np.asarray(xi, dtype=LD)
    if kind == "TET4":     # the simplex (-1,-1,-1), (1,-1,-1), (-1,1,-1), (-1,-1,1)
        return np.array([[-0.5, -0.5, -0.5], [0.5, 0.0, 0.0], [0.0, 0.5, 0.0], [0.0, 0.0, 0.5]], dtype=LD)
    sg = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], dtype=LD)
    t = 1 + sg * xi
    return np.stack([sg[:, 0] * t[:, 1] * t[:, 2], t[:, 0] * sg[:, 1] * t[:, 2], t[:, 0] * t[:, 1] * sg[:, 2]], axis=1) / 8


def _shape_values(kind, xi):
    xi = np.asarray(xi, dtype=LD)
    if kind == "TET4":
        return np.array([-(1 + xi.sum()) / 2, (1 + xi[0]) / 2, (1 + xi[1]) / 2, (1 + xi[2]) / 2], dtype=LD)
    sg = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], dtype=LD)
    return np.prod(1 + sg * xi, axis=1) / 8


def _inverse3(J):
    c = np.array([[J[1, 1] * J[2, 2] - J[1, 2] * J[2, 1], J[0, 2] * J[2, 1] - J[0, 1] * J[2, 2], J[0, 1] * J[1, 2] - J[0, 2] * J[1, 1]],
                  [J[1, 2] * J[2, 0] - J[1, 0] * J[2, 2], J[0, 0] * J[2, 2] - J[0, 2] * J[2, 0], J[0, 2] * J[1, 0] - J[0, 0] * J[1, 2]],
                  [J[1, 0] * J[2, 1] - J[1, 1] * J[2, 0], J[0, 1] * J[2, 0] - J[0, 0] * J[2, 1], J[0, 0] * J[1, 1] - J[0, 1] * J[1, 0]]], dtype=LD)
    det = J[0, 0] * c[0, 0] + J[0, 1] * c[1, 0] + J[0, 2] * c[2, 0]
    return c / det, det


class LongDoubleElastic:
    """M a + K u + g(u) = lf f with LinearElastic on a 3-D Hex8 or Tet4 mesh and the penalty contact term, everything in np.longdouble: the
    interface of dr.Problem with cr.ContactMixin as far as the functions of this module use it.  groups: [(connectivity, weights, points)]"""

    dtype = LD

    def __init__(self, kind, vertices, groups, mu, lam, rho=1.0, f=None, obstacles=(), node_weights=None):
        self.vertices = np.asarray(vertices, dtype=np.float64)
        X = self.vertices.astype(LD)
        self.N, self.d = X.shape
        self.s, self.n = 3, 3 * self.N
        self.free = np.ones(self.n, dtype=bool)
        self.f = np.zeros(self.n, dtype=LD) if f is None else np.asarray(f, dtype=LD).reshape(-1)
        self.obstacles, self.node_weights = list(obstacles), node_weights
        mu, lam, rho = LD(mu), LD(lam), LD(rho)
        K, M = np.zeros((self.n, self.n), dtype=LD), np.zeros((self.n, self.n), dtype=LD)
        eye = np.eye(3, dtype=LD)
        for conn, w, p in groups:
            for el in np.asarray(conn, dtype=np.int64):
                Xe = X[el]
                ke, me = np.zeros((3 * len(el),) * 2, dtype=LD), np.zeros((len(el),) * 2, dtype=LD)
                for wq, xq in zip(np.asarray(w, dtype=LD), np.asarray(p)):
                    dN = _shape_gradients(kind, xq)
                    Jinv, det = _inverse3(Xe.T @ dN)           # J[a][b] = dx_a / dxi_b
                    G = dN @ Jinv                               # dN_i / dx_a
                    wd = wq * abs(det)
                    # K[(i,a),(j,b)] = mu (G_i . G_j delta_ab + G_ib G_ja) + lam G_ia G_jb
                    GG = G @ G.T
                    ke += wd * (mu * (np.einsum("ij,ab->iajb", GG, eye) + np.einsum("ib,ja->iajb", G, G)) + lam * np.einsum("ia,jb->iajb", G, G)).reshape(ke.shape)
                    Nv = _shape_values(kind, xq)
                    me += wd * rho * np.outer(Nv, Nv)
                dofs = (3 * el[:, None] + np.arange(3)).reshape(-1)
                K[np.ix_(dofs, dofs)] += ke
                for a in range(3):
                    M[np.ix_(3 * el + a, 3 * el + a)] += me
        self.K, self.M = K, M

    def lf(self, n):
        return 1.0

    def mass(self):
        return self.M

    def lumped(self):
        return self.M @ np.ones(self.n, dtype=LD)

    def contact_force(self, u):
        X = self.vertices
        x = X.astype(LD) + np.asarray(u, dtype=LD).reshape(X.shape)
        w = np.ones(self.N, dtype=LD) if self.node_weights is None else np.asarray(self.node_weights, dtype=LD)
        g = np.zeros(X.shape, dtype=LD)
        for ob in self.obstacles:
            for i in range(self.N):
                phi, n = _eval(ob, x[i], LD)
                if phi < 0 and n is not None:
                    g[i] += LD(ob[3]) * w[i] * phi * n
        return g.reshape(-1)

    def residual(self, u):
        return self.K @ np.asarray(u, dtype=LD) + self.contact_force(u)

    def tangent(self, u):
        """float64: it only steers Newton's steps"""
        return sp.csr_matrix(self.K.astype(np.float64)) + cr.tangent(self.obstacles, self.vertices, np.asarray(u, dtype=np.float64), self.node_weights)

    def solve_free(self, A, b):
        """A x = b on the free dofs: a float64 factorisation, refined in long double until the correction is below its rounding"""
        A = A.toarray() if sp.issparse(A) else np.asarray(A)
        fr = self.free
        Ald, A64 = A[np.ix_(fr, fr)].astype(LD), A[np.ix_(fr, fr)].astype(np.float64)
        b = np.asarray(b, dtype=LD)[fr]
        x = np.zeros(len(b), dtype=LD)
        for _ in range(6):
            x = x + np.linalg.solve(A64, (b - Ald @ x).astype(np.float64)).astype(LD)
        out = np.zeros(self.n, dtype=LD)
        out[fr] = x
        return out


def newton_ld(prob, F, J, u, tol, max_it=60):
    """dr.newton's iteration (backtracking rule included) on long-double iterates; J in float64 steers the steps"""
    u = np.array(u, dtype=LD)
    Fu = F(u)
    it = 0
    while True:
        fn = np.sqrt(Fu @ Fu)
        if not np.isfinite(fn):
            return "nonfinite", u, it
        if fn <= tol:
            return "ok", u, it
        if it == max_it:
            return "maxit", u, it
        step = -prob.solve_free(J(u), Fu)
        g0, a_prev, a = fn * fn / 2, 0.0, 1.0
        while True:
            u = u + LD(a - a_prev) * step
            Fu = F(u)
            if (Fu @ Fu) / 2 <= (1.0 - 1e-4 * a) * g0:
                break
            if a < 1e-6:
                return "line_search", u, it
            a_prev, a = a, {1.0: 0.75, 0.75: 0.5, 0.5: 0.25}.get(a, 0.25 * a)
        it += 1


class StableProblem(cr.ContactMixin, dr.Problem):
    """the problem on the long-double reference of the Stable Neo-Hookean law (stable_neo_hookean_reference), rounded to double, with the
    contact term: what dr.newton and the integrators need"""

    def __init__(self, kind, vertices, conn, w, p, lame, rho=1.0, f=None, obstacles=(), node_weights=None):
        import stable_neo_hookean_reference as snh

        self.snh, self.conn = snh, np.asarray(conn)
        self.kind, self.vertices, self.w, self.p, self.lame, self.rho = kind, np.asarray(vertices), w, p, lame, rho
        self.d = self.s = self.vertices.shape[1]
        self.N = len(self.vertices)
        self.n = self.s * self.N
        self.free = np.ones(self.n, dtype=bool)
        self.f = np.zeros(self.n) if f is None else np.asarray(f, dtype=np.float64).reshape(-1)
        self.load_factor, self.direct, self._mass = None, "dense", None
        self.set_contact(obstacles, node_weights)

    def ref(self, u):
        return self.snh.Reference(self.kind, self.vertices, self.conn, self.w, self.p, u, self.lame.mu, self.lame.lambda_, rho=self.rho)

    def _base_residual(self, u):
        return self.ref(u).residual().astype(np.float64)

    def _base_energy(self, u):
        return float(self.ref(u).energy())

    def _base_tangent(self, u):
        ref = self.ref(u)
        ro, ci = ref.pattern()
        return sp.csr_matrix((ref.csr_values(ro, ci, "K").astype(np.float64), ci, ro), shape=(self.n, self.n))
