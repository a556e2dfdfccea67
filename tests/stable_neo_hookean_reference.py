"""The Stable Neo-Hookean law (FH_STABLE_NEO_HOOKEAN) in extended precision, as a `hp_reference.Reference`.

Written from the formulas of include/fenris_hip.h alone and sharing no code with the library: the cofactor matrix by its minors, its derivative
from the definition  d cof F[i][j] / d F[k][l] = eps_ikm eps_jln F[m][n]  (d = 3) or  eps_ik eps_jl  (d = 2) with the permutation symbol, the
logarithm in the working type.  gamma = det F - 1 is taken as det(F) - 1 in long double: the cancellation costs ~1e-19 there, so the reference
does not share the device's expansion either.

    psi = mu/2 [c - log1p(c / (d + 1))] + lambda/2 gamma^2 - k gamma,   c = F:F - d,  k = mu d / (d + 1)
    P   = mu (1 - 1/(d + 1 + c)) F + (lambda gamma - k) cof F

`Reference(kind, ...)` is `hp_reference.Reference` with this law in place of its three (the geometry, the sums and the scales are that class's,
unedited); it also keeps det_F_max, so that a test can assert that both signs of det F occur."""
import numpy as np

import hp_reference as hp

MODEL = "STABLE_NEO_HOOKEAN"


def _eps(d, dt):
    e = np.zeros((d,) * d, dtype=dt)
    if d == 2:
        e[0, 1], e[1, 0] = 1, -1
    else:
        for i, j, k in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
            e[i, j, k], e[i, k, j] = 1, -1
    return e


def cofactor(F):
    """cof F = dJ/dF of a stack (E, d, d), by minors"""
    C = np.empty_like(F)
    d = F.shape[-1]
    if d == 2:
        C[:, 0, 0], C[:, 0, 1], C[:, 1, 0], C[:, 1, 1] = F[:, 1, 1], -F[:, 1, 0], -F[:, 0, 1], F[:, 0, 0]
        return C
    for i in range(3):
        for j in range(3):
            r = [k for k in range(3) if k != i]
            c = [k for k in range(3) if k != j]
            C[:, i, j] = (-1) ** (i + j) * (F[:, r[0], c[0]] * F[:, r[1], c[1]] - F[:, r[0], c[1]] * F[:, r[1], c[0]])
    return C


def parameters(d, mu_lame, lambda_lame):
    """the law's (mu, lambda) that linearise at F = I to the Lame pair (closed form of fh_stable_neo_hookean_parameters)"""
    return (d + 1.0) / d * mu_lame, lambda_lame + mu_lame - 2.0 * mu_lame / (d * (d + 1.0))


def stress(F, mu, lam, I):
    """P (E, d, d), psi (E,) and the magnitudes of their terms, the shapes of hp_reference._stress"""
    d = F.shape[-1]
    dt = F.dtype.type
    ff = np.einsum("eij,eij->e", F, F)
    c = ff - d
    gamma = hp.det(F) - 1
    k = mu * (dt(d) / dt(d + 1))
    m = d + 1 + c
    C = cofactor(F)
    a0 = mu * ((d + c) / m)              # = mu (1 - 1/m), in the form in which a0 = k at F = I exactly
    b = lam * gamma - k
    P = a0[:, None, None] * F + b[:, None, None] * C
    lg = np.log1p(c / dt(d + 1))
    psi = mu / 2 * (c - lg) + lam / 2 * gamma ** 2 - k * gamma
    P_abs = (mu * (1 + 1 / m))[:, None, None] * np.abs(F) + (lam * np.abs(gamma) + k)[:, None, None] * np.abs(C)
    psi_abs = mu / 2 * (ff + d + np.abs(lg)) + lam / 2 * gamma ** 2 + k * np.abs(gamma)
    return P, psi, P_abs, psi_abs


def contraction(F, g, mu, lam, I):
    """the element blocks C(g_a, g_b)[i][j] of one point as an array (E, a, i, b, j), the shape of hp_reference._contraction"""
    d = F.shape[-1]
    dt = F.dtype.type
    c = np.einsum("eij,eij->e", F, F) - d
    gamma = hp.det(F) - 1
    m = d + 1 + c
    a0 = mu * ((d + c) / m)
    a1 = 2 * mu / m ** 2
    b = lam * gamma - mu * (dt(d) / dt(d + 1))
    gg = np.einsum("eak,ebk->eab", g, g)
    Fg = np.einsum("eik,eak->eai", F, g)
    Cg = np.einsum("eik,eak->eai", cofactor(F), g)
    e = _eps(d, dt)
    if d == 3:
        G = np.einsum("ikm,jln,eaj,ebl,emn->eaibk", e, e, g, g, F)
    else:
        G = np.einsum("ik,jl,eaj,ebl->eaibk", e, e, g, g)
    s = (slice(None), None, None, None, None)
    return (a0[s] * gg[:, :, None, :, None] * I[None, None, :, None, :] + a1[s] * np.einsum("eai,ebj->eaibj", Fg, Fg)
            + np.reshape(lam, (-1, 1, 1, 1, 1)) * np.einsum("eai,ebj->eaibj", Cg, Cg) + b[s] * G)


class Reference(hp.Reference):
    """hp_reference.Reference for this law: the same constructor without `model`; mu, lam are the law's own parameters.  per_point: (E, nq, 2)
    parameters of every element and point instead (a compact table written out)."""

    def __init__(self, kind, vertices, connectivity, weights, points, u, mu, lam, rho=1.0, dt=np.longdouble, per_point=None):
        self.det_F_max = -np.inf
        calls = {"stress": 0, "contraction": 0}   # the base class visits the points in order, the stress and then the contraction of each

        def params(which, mu_, lam_):
            q = calls[which]
            calls[which] += 1
            if per_point is None:
                return mu_, lam_
            pq = np.asarray(per_point, dtype=np.float64)[:, q, :].astype(dt)
            return pq[:, 0], pq[:, 1]

        def _stress(model, F, mu_, lam_, I):
            self.det_F_max = max(self.det_F_max, float(hp.det(F).max()))
            return stress(F, *params("stress", mu_, lam_), I)

        def _contraction(model, F, g, mu_, lam_, I):
            return contraction(F, g, *params("contraction", mu_, lam_), I)

        saved = hp._stress, hp._contraction   # the base class looks its law up by these module names
        hp._stress, hp._contraction = _stress, _contraction
        try:
            super().__init__(kind, MODEL, vertices, connectivity, weights, points, u, mu, lam, rho=rho, dt=dt)
        finally:
            hp._stress, hp._contraction = saved


def at_points(kind, vertices, connectivity, points, u, mu, lam, dt=np.longdouble):
    """per (element, point), in the order of the quadrature points: grad u (d, s) with g[i][k] = d u_k / d x_i, F, P, psi and the magnitudes of
    the terms of P and psi -- what recovery returns at the points"""
    n, d = hp.KINDS[kind]
    X = np.asarray(vertices, dtype=np.float64).astype(dt)
    conn = np.asarray(connectivity).astype(np.int64)
    gkind = hp.GEOMETRY.get(kind, kind)
    Xe, Ue = X[conn[:, :hp.KINDS[gkind][0]]], np.asarray(u, dtype=np.float64).reshape(-1, d).astype(dt)[conn]
    I = np.eye(d, dtype=dt)
    out = {k: [] for k in ("grad_u", "F", "P", "psi", "P_abs", "psi_abs")}
    for xi in np.asarray(points, dtype=np.float64).reshape(-1, d):
        _, G = hp.shape(kind, xi, dt)
        _, Gg = hp.shape(gkind, xi, dt)
        g = np.einsum("nk,ekj->enj", G, hp.inv(np.einsum("eni,nj->eij", Xe, Gg)))
        gu = np.einsum("eni,enk->eik", g, Ue)
        F = I + np.swapaxes(gu, 1, 2)
        P, psi, P_abs, psi_abs = stress(F, dt(float(mu)), dt(float(lam)), I)
        for k, v in zip(out, (gu, F, P, psi, P_abs, psi_abs)):
            out[k].append(v)
    return {k: np.stack(v, axis=1).reshape((-1,) + v[0].shape[1:]) for k, v in out.items()}
