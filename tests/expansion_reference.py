"""The per-element expansion (fh_set_element_expansion) in extended precision, as a `hp_reference.Reference`.

theta_e > 0 is the isotropic stress-free stretch of element e.  The law is written here at the level of grad u at a quadrature point, from
include/fenris_hip.h alone -- not through nodal values, so it does not share the form the register-resident kernels take it in.  With
F = I + (grad u)^T the total deformation gradient that the base class hands to its material functions:

    LINEAR_ELASTIC (additive small strain)   gu_e = gu - (theta - 1) I, i.e. F_e = F - (theta - 1) I;
                                             P = P_0(F_e), psi = psi_0(F_e), the contraction (the tangent) unchanged
    NEO_HOOKEAN, STVK, STABLE_NEO_HOOKEAN    gu_e = (gu - (theta - 1) I) / theta, i.e. F_e = F / theta (F = F_e theta);
                                             psi = theta^d psi_0(F_e), P = theta^(d-1) P_0(F_e), contraction = theta^(d-2) C_0(F_e)

`Reference(kind, model, ..., theta)` is `hp_reference.Reference` with these in place of its material functions for the length of the
constructor (the geometry, the sums and the scales are that class's, unedited; the Stable Neo-Hookean law is the one of
stable_neo_hookean_reference.py).  It adds the quadratic kinds the base class lacks -- TRI6, QUAD9, HEX20, written out from their
definitions -- and a dense solve of the linear problem K u = f_th on the free dofs."""
import numpy as np

import hp_reference as hp
import stable_neo_hookean_reference as snh

MODELS = ("LINEAR_ELASTIC", "NEO_HOOKEAN", "STVK", "STABLE_NEO_HOOKEAN")
QUAD9_NODES = np.array([(-1, -1), (1, -1), (1, 1), (-1, 1), (0, -1), (1, 0), (0, 1), (-1, 0), (0, 0)])
TRI6_EDGES = [(0, 1), (1, 2), (0, 2)]   # nodes 3 .. 5: the midpoints of these vertex pairs
EXTRA_KINDS = {"TRI6": (6, 2), "QUAD9": (9, 2), "HEX20": (20, 3)}
EXTRA_GEOMETRY = {"TRI6": "TRI3", "QUAD9": "QUAD4", "HEX20": "HEX8"}


def shape(kind, xi, dt=np.longdouble):
    """hp_reference.shape with TRI6, QUAD9 (tensor products of the quadratic Lagrange factors) and HEX20 (serendipity: corners
    (1 + a x)(1 + b y)(1 + c z)(a x + b y + c z - 2) / 8, the mid-edge node of an edge along x (1 - x^2)(1 + b y)(1 + c z) / 4)"""
    if kind not in EXTRA_KINDS:
        return _base_shape(kind, xi, dt)
    xi = np.asarray(xi, dtype=np.float64).astype(dt)
    if kind == "TRI6":
        lam, dl = hp._simplex(xi, dt)
        phi, g = np.empty(6, dtype=dt), np.empty((6, 2), dtype=dt)
        phi[:3] = lam * (2 * lam - 1)
        g[:3] = (4 * lam - 1)[:, None] * dl
        for m, (i, j) in enumerate(TRI6_EDGES):
            phi[3 + m] = 4 * lam[i] * lam[j]
            g[3 + m] = 4 * (lam[i] * dl[j] + lam[j] * dl[i])
        return phi, g
    if kind == "QUAD9":
        nodes = QUAD9_NODES.astype(dt)
        x = xi[None, :]
        v = np.where(nodes == 0, 1 - x * x, x * (x + nodes) / 2)
        dv = np.where(nodes == 0, -2 * x, x + nodes / 2)
        return v[:, 0] * v[:, 1], np.stack([dv[:, 0] * v[:, 1], v[:, 0] * dv[:, 1]], axis=1)
    nodes = hp.HEX27_NODES[:20].astype(dt)   # HEX20: the corners and the twelve mid-edge nodes of Hex27, in its order
    phi, g = np.empty(20, dtype=dt), np.empty((20, 3), dtype=dt)
    for n, s in enumerate(nodes):
        lin = 1 + s * xi                     # the factor of an axis the node is at an end of
        if n < 8:
            f = np.dot(s, xi) - 2
            p = lin[0] * lin[1] * lin[2]
            phi[n] = p * f / 8
            for k in range(3):
                g[n, k] = (s[k] * np.prod(np.delete(lin, k)) * f + p * s[k]) / 8
        else:
            k0 = int(np.argmax(s == 0))      # the axis of the edge
            fac = [1 - xi[k] * xi[k] if k == k0 else lin[k] for k in range(3)]
            dfac = [-2 * xi[k] if k == k0 else s[k] for k in range(3)]
            phi[n] = fac[0] * fac[1] * fac[2] / 4
            for k in range(3):
                g[n, k] = dfac[k] * np.prod([fac[j] for j in range(3) if j != k]) / 4
    return phi, g


_base_shape = hp.shape


def stretches(theta, num_elements, dt=np.longdouble):
    th = np.asarray(theta, dtype=np.float64).reshape(-1)
    assert len(th) in (1, num_elements), "theta: one value or one per element"
    return np.broadcast_to(th.astype(dt), (num_elements,))


def thermal_stretches(connectivity, T, alpha, T_ref, dt=np.float64):
    """theta_e = 1 + alpha_e (mean of the nodal temperatures, summed in local node order, - T_ref), in doubles as the device forms it"""
    conn = np.asarray(connectivity).astype(np.int64)
    T = np.asarray(T, dtype=dt)
    total = np.zeros(len(conn), dtype=dt)
    for a in range(conn.shape[1]):
        total = total + T[conn[:, a]]
    al = np.broadcast_to(np.asarray(alpha, dtype=dt).reshape(-1), (len(conn),))
    return 1.0 + al * (total / dt(conn.shape[1]) - dt(T_ref))


class Reference(hp.Reference):
    """hp_reference.Reference under the expansion theta (one value, or one per element); model: one of MODELS (STABLE_NEO_HOOKEAN takes the
    law's own parameters, as stable_neo_hookean_reference.Reference does)."""

    def __init__(self, kind, model, vertices, connectivity, weights, points, u, mu, lam, theta, rho=1.0, dt=np.longdouble):
        assert model in MODELS
        E = len(connectivity)
        th = stretches(theta, E, dt)
        d = (hp.KINDS.get(kind) or EXTRA_KINDS[kind])[1]
        base_stress = (lambda m, F, a, b, I: snh.stress(F, a, b, I)) if model == "STABLE_NEO_HOOKEAN" else hp._stress
        base_contraction = (lambda m, F, g, a, b, I: snh.contraction(F, g, a, b, I)) if model == "STABLE_NEO_HOOKEAN" else hp._contraction
        t3 = th[:, None, None]

        def power(k):   # theta^k by multiplication
            out = np.ones(E, dtype=dt)
            for _ in range(k):
                out = out * th
            return out

        def _stress(m, F, a, b, I):
            if model == "LINEAR_ELASTIC":
                return base_stress(m, F - (t3 - 1) * I, a, b, I)
            P, psi, P_abs, psi_abs = base_stress(m, F / t3, a, b, I)
            sP, sPsi = power(d - 1), power(d)
            return sP[:, None, None] * P, sPsi * psi, sP[:, None, None] * P_abs, sPsi * psi_abs

        def _contraction(m, F, g, a, b, I):
            if model == "LINEAR_ELASTIC":
                return base_contraction(m, F, g, a, b, I)
            return power(d - 2)[:, None, None, None, None] * base_contraction(m, F / t3, g, a, b, I)

        saved = hp._stress, hp._contraction, hp.shape, dict(hp.KINDS), dict(hp.GEOMETRY)   # the base class looks these up by module name
        hp._stress, hp._contraction, hp.shape = _stress, _contraction, shape
        hp.KINDS.update(EXTRA_KINDS)
        hp.GEOMETRY.update(EXTRA_GEOMETRY)
        try:
            super().__init__(kind, model, vertices, connectivity, weights, points, u, mu, lam, rho=rho, dt=dt)
        finally:
            hp._stress, hp._contraction, hp.shape = saved[:3]
            hp.KINDS.clear(); hp.KINDS.update(saved[3])
            hp.GEOMETRY.clear(); hp.GEOMETRY.update(saved[4])
        self.theta = th

    def dense_k(self):
        """K as a dense (ndof, ndof) array of doubles"""
        rows, cols = np.divmod(self.pattern_keys, self.ndof)
        K = np.zeros((self.ndof, self.ndof))
        K[rows, cols] = self._on_pattern(self.ke).astype(np.float64)
        return K

    def thermal_load(self):
        """f_th = -r(0); this object must have been built at u = 0"""
        return -self.residual()

    def solve_linear(self, fixed_dofs, f=None):
        """the solution of K u = f + f_th on the free dofs, zero on the fixed ones (LINEAR_ELASTIC, built at u = 0), by a dense solve in doubles"""
        assert self.model == "LINEAR_ELASTIC"
        rhs = self.thermal_load().astype(np.float64) + (0.0 if f is None else np.asarray(f, dtype=np.float64))
        free = np.setdiff1d(np.arange(self.ndof), np.asarray(fixed_dofs, dtype=np.int64))
        u = np.zeros(self.ndof)
        u[free] = np.linalg.solve(self.dense_k()[np.ix_(free, free)], rhs[free])
        return u
