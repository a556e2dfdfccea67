"""NumPy statement of the augmented-Lagrangian contact term of fh_set_contact_multipliers / fh_contact_multiplier_update
(include/fenris_hip.h), for tests/test_augmented_contact.py, on top of contact_reference.py, friction_reference.py, sdf_grid_reference.py
and dynamics_reference.py (all imported unchanged; sdf_grid_reference puts its dispatcher in front of contact_reference.phi_grad_hess, so
obstacle lists may hold "grid" and "curved" tuples beside the three analytic kinds).

The multiplier of obstacle o and node i is a length s[o, i] >= 0 standing for the force lam = k_o w_i s[o, i].  With
    phi_eff = phi_o(x_i) - s[o, i],   p = min(0, phi_eff)
    E_c = sum (k w / 2) (p^2 - s^2)
    g_i = sum k w p n
    B_i = sum k w ([phi_eff < 0] n n^T + p Hess phi)            (exact=True: the derivative of g with s frozen)
    B_i = sum k w ([phi_eff < 0] n n^T + max-PSD(p Hess phi))   (exact=False: what the library applies; a grid drops p Hess phi whole)
    friction: in contact at xbar iff phi_eff(xbar) < 0, lam = k w max(0, -phi_eff(xbar)) (a grid: times |m|, nbar = m / |m|)
    update:  s <- max(0, s - phi_o(x_i));  phi = +inf (outside a grid's box) gives 0
A node without a gradient (the centre of a ball or cavity, a grid's flat spot or outside its box) gets no force and no block; its energy
counts.  `s` None is all zeros, and then every function returns contact_reference's / sdf_grid_reference's value, array_equal."""
import numpy as np
import scipy.sparse as sp

import contact_reference as cr
import dynamics_reference as dr
import friction_reference as fr
import sdf_grid_reference as sg


def multipliers(obstacles, X, s=None):
    """s as an array of shape (len(obstacles), N); None: zeros"""
    shape = (len(obstacles), len(X))
    return np.zeros(shape) if s is None else np.asarray(s, dtype=np.float64).reshape(shape)


def _weights(X, w):
    return np.ones(len(X)) if w is None else np.asarray(w, dtype=np.float64)


def energy(obstacles, X, u, s=None, w=None):
    x, s, w = cr.positions(X, u), multipliers(obstacles, X, s), _weights(X, w)
    e = 0.0
    for o, ob in enumerate(obstacles):
        for i, xi in enumerate(x):
            phi = cr.phi_grad_hess(ob, xi)[0] - s[o, i]
            if phi < 0.0:
                e += 0.5 * ob[3] * w[i] * phi * phi
            e -= 0.5 * ob[3] * w[i] * s[o, i] * s[o, i]
    return e


def force(obstacles, X, u, s=None, w=None):
    x, s, w = cr.positions(X, u), multipliers(obstacles, X, s), _weights(X, w)
    g = np.zeros_like(x)
    for o, ob in enumerate(obstacles):
        for i, xi in enumerate(x):
            phi, n, _ = cr.phi_grad_hess(ob, xi)
            phi = phi - s[o, i]
            if phi < 0.0 and n is not None:
                g[i] += ob[3] * w[i] * phi * n
    return g.reshape(-1)


def blocks(obstacles, X, u, s=None, w=None, exact=False):
    x, s, w = cr.positions(X, u), multipliers(obstacles, X, s), _weights(X, w)
    d = x.shape[1]
    B = np.zeros((len(x), d, d))
    for o, ob in enumerate(obstacles):
        for i, xi in enumerate(x):
            phi, n, H = cr.phi_grad_hess(ob, xi)
            phi = phi - s[o, i]
            if phi < 0.0 and n is not None:
                curv = phi * H
                if not exact:
                    curv = 0.0 if ob[0] in sg.SAMPLED else cr._psd_part(curv)
                B[i] += ob[3] * w[i] * (np.outer(n, n) + curv)
    return B


def tangent(obstacles, X, u, s=None, w=None, exact=False):
    return sp.block_diag(list(blocks(obstacles, X, u, s, w, exact)), format="csr")


def resultants(obstacles, X, u, s=None, w=None):
    """R[o]: obstacle o's share of g"""
    s = multipliers(obstacles, X, s)
    return np.array([force([ob], X, u, s[o:o + 1], w).reshape(np.shape(X)).sum(axis=0) for o, ob in enumerate(obstacles)])


def _gradient_norm(ob, xi):
    if ob[0] not in sg.SAMPLED:
        return 1.0
    m = cr.phi_grad_hess(ob, xi)[1]
    return 0.0 if m is None else float(np.sqrt(m @ m))


def multiplier_forces(obstacles, X, u, s=None, w=None):
    """lam[o, i] = k w s, a grid: times |grad phi| at the current position (0 outside its box)"""
    x, s, w = cr.positions(X, u), multipliers(obstacles, X, s), _weights(X, w)
    return np.array([[ob[3] * w[i] * s[o, i] * _gradient_norm(ob, xi) for i, xi in enumerate(x)] for o, ob in enumerate(obstacles)])


def update(obstacles, X, u, s=None, w=None, skip=()):
    """(s_new, stats): stats = dict(max_change, max_penetration, active, max_force) over the pairs of the nodes not in `skip`, which keep 0"""
    s = multipliers(obstacles, X, s)
    phi = cr.phi_table(obstacles, X, u)
    with np.errstate(invalid="ignore"):
        new = np.maximum(0.0, s - phi)
    skip = np.asarray(skip, dtype=np.int64)
    new[:, skip] = 0.0
    counted = np.ones(len(X), dtype=bool)
    counted[skip] = False
    lam = multiplier_forces(obstacles, X, u, new, w)
    c = counted
    fin = np.isfinite(phi) & c[None, :]
    margin = float(np.abs(s - np.where(fin, phi, 0.0))[fin].min(initial=np.inf))     # how far the nearest counted pair is from switching
    stats = dict(margin=margin, max_change=float(np.abs(new - s)[:, c].max(initial=0.0)), max_penetration=float(np.maximum(0.0, -phi)[:, c].max(initial=0.0)),
                 active=int((new[:, c] > 0.0).sum()), max_force=float(lam[:, c].max(initial=0.0)))
    return new, stats


# ---- friction with the multipliers standing
def _friction_visit(obstacles, mu, X, ubar, d, s, w):
    """yields (node, mu lam, nbar, slip, |slip|) for every pair in contact at the lag position: phi_eff(xbar) < 0"""
    X = np.asarray(X, dtype=np.float64)
    xbar = X + np.asarray(ubar, dtype=np.float64).reshape(X.shape)
    d = np.asarray(d, dtype=np.float64).reshape(X.shape)
    s, w = multipliers(obstacles, X, s), _weights(X, w)
    for o, (ob, m) in enumerate(zip(obstacles, mu)):
        if not m > 0.0:
            continue
        for i in range(len(X)):
            phi, n, _ = cr.phi_grad_hess(ob, xbar[i])
            phi = phi - s[o, i]
            if not phi < 0.0 or n is None:
                continue
            gn = 1.0
            if ob[0] in sg.SAMPLED:
                gn = float(np.sqrt(n @ n))
                n = n / gn
            slip = d[i] - n * (n @ d[i])
            yield i, m * (ob[3] * w[i] * -phi * gn), n, slip, float(np.sqrt(slip @ slip))


def friction_potential(obstacles, mu, X, ubar, d, eps, s=None, w=None):
    return sum((ml * fr._coefficients(y, eps)[0] for _, ml, _, _, y in _friction_visit(obstacles, mu, X, ubar, d, s, w)), 0.0)


def friction_force(obstacles, mu, X, ubar, d, eps, s=None, w=None):
    q = np.zeros(np.shape(X))
    for i, ml, _, slip, y in _friction_visit(obstacles, mu, X, ubar, d, s, w):
        q[i] += ml * fr._coefficients(y, eps)[1] * slip
    return q.reshape(-1)


def friction_blocks(obstacles, mu, X, ubar, d, eps, s=None, w=None):
    N, dim = np.shape(X)
    H = np.zeros((N, dim, dim))
    for i, ml, n, slip, y in _friction_visit(obstacles, mu, X, ubar, d, s, w):
        _, c1, c2 = fr._coefficients(y, eps)
        H[i] += ml * (c1 * (np.eye(dim) - np.outer(n, n)) - c2 * np.outer(slip, slip))
    return H


def friction_resultants(obstacles, mu, X, ubar, d, eps, s=None, w=None):
    s = multipliers(obstacles, X, s)
    return np.array([friction_force([ob], [mu[o]], X, ubar, d, eps, s[o:o + 1], w).reshape(np.shape(X)).sum(axis=0) for o, ob in enumerate(obstacles)])


# ---- the problem with the shifted law, and the outer loop
class AugmentedProblem:
    """wraps a contact problem (cr.ContactMixin on dr.Problem): residual, energy and tangent with the multipliers `s` frozen, and, with
    `mu`, the friction term at the lag state (ubar, eps); everything else is the wrapped problem's, so dr.newton, dr.central_difference,
    dr.implicit and dr.power_iteration work on it unchanged"""

    def __init__(self, prob, s=None, mu=None, eps=None, ubar=None):
        self.prob = prob
        self.s = multipliers(prob.obstacles, prob.vertices, s)
        self.mu, self.eps = mu, eps
        self.ubar = np.zeros(prob.n) if ubar is None else np.array(ubar, dtype=np.float64)

    def __getattr__(self, name):
        return getattr(self.prob, name)

    def _c(self):
        return self.prob.obstacles, self.prob.vertices

    def _fargs(self, u):
        return self.prob.obstacles, self.mu, self.prob.vertices, self.ubar, np.asarray(u) - self.ubar, self.eps, self.s, self.prob.node_weights

    def contact_force(self, u):
        return force(*self._c(), u, self.s, self.prob.node_weights)

    def contact_energy(self, u):
        return energy(*self._c(), u, self.s, self.prob.node_weights)

    def residual(self, u):
        r = self.prob._base_residual(u) + self.contact_force(u)
        return r + friction_force(*self._fargs(u)) if self.mu is not None else r

    def energy(self, u):
        return self.prob._base_energy(u) + self.contact_energy(u)

    def tangent(self, u):
        K = self.prob._base_tangent(u) + tangent(*self._c(), u, self.s, self.prob.node_weights, getattr(self.prob, "exact", False))
        if self.mu is not None:
            K = K + sp.block_diag(list(friction_blocks(*self._fargs(u))), format="csr")
        return K.tocsr()

    def update(self, u, skip=()):
        self.s, stats = update(*self._c(), u, self.s, self.prob.node_weights, skip)
        return stats


def static_newton(aug, f, u0, tol, max_it=60):
    """dr.newton on r + g (+ q) = f with the multipliers of `aug` frozen: (status, u, iterations)"""
    fr_ = aug.free

    def F(x):
        out = aug.residual(x) - f
        out[~fr_] = 0.0
        return out

    return dr.newton(aug, F, aug.tangent, np.array(u0, dtype=np.float64), tol, True, max_it)


def augmented_lagrangian(aug, f, u0, newton_tol, max_updates=30, tol=1e-10, skip=()):
    """the outer loop: Newton with s frozen, update at the solution, until max_change <= tol.  Returns (u, history, converged); history holds
    per update a dict with the update's statistics, the Newton iterations, the active set (s_new > 0) and a copy of u"""
    u = np.array(u0, dtype=np.float64)
    history = []
    for _ in range(max_updates):
        st, u, it = static_newton(aug, f, u, newton_tol)
        assert st == "ok", st
        stats = aug.update(u, skip)
        stats.update(newton_iterations=it, active_set=aug.s > 0.0, u=u.copy())
        history.append(stats)
        if stats["max_change"] <= tol:
            return u, history, True
    return u, history, False
