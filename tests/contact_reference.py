"""NumPy statement of the penalty contact term of fh_set_obstacles (include/fenris_hip.h), for tests/test_contact.py.

Obstacle o has a signed distance phi_o, positive where the body may be, and a stiffness k_o.  With x_i = X_i + u_i, w_i a node weight and
p = min(0, phi_o(x_i)):
    E_c = sum_o sum_i (k_o w_i / 2) p^2
    g_i = sum_o k_o w_i p grad phi_o(x_i)
    B_i = sum_o k_o w_i ([phi_o < 0] n n^T + p Hess phi_o)                    (exact=True: the derivative of g)
    B_i = sum_o k_o w_i ([phi_o < 0] n n^T + max-PSD(p Hess phi_o))           (exact=False: what the library applies)
p Hess phi is zero for the half-space, negative semi-definite for the ball (dropped by the rule) and positive semi-definite for the cavity
(kept).  A node at the centre of a ball or cavity has no gradient: no force, no block, but its energy counts.  The test phi < 0 is strict.

An obstacle is a tuple: ("half_space", point, normal, k), ("ball", centre, radius, k) or ("cavity", centre, radius, k).
ContactProblem is dynamics_reference.Problem with the term added to residual, energy and tangent, so that dr.newton,
dr.central_difference, dr.implicit, dr.power_iteration and dr.dense_pencil work on it unchanged."""
import numpy as np
import scipy.sparse as sp

import dynamics_reference as dr


def phi_grad_hess(ob, x):
    """(phi, n or None, Hess phi or None) of one obstacle at the point x (d entries)"""
    kind, p, q, _ = ob
    d = len(x)
    p = np.asarray(p, dtype=np.float64)[:d]
    if kind == "half_space":
        n = np.asarray(q, dtype=np.float64)[:d]
        n = n / np.linalg.norm(n)
        return float((x - p) @ n), n, np.zeros((d, d))
    y = x - p
    r = float(np.sqrt(y @ y))
    sign = 1.0 if kind == "ball" else -1.0
    phi = sign * (r - float(q))
    if r == 0.0:
        return phi, None, None
    yh = y / r
    return phi, sign * yh, sign * (np.eye(d) - np.outer(yh, yh)) / r


def _psd_part(A):
    w, V = np.linalg.eigh(0.5 * (A + A.T))
    return (V * np.maximum(w, 0.0)) @ V.T


def positions(X, u):
    X = np.asarray(X, dtype=np.float64)
    return X + np.asarray(u, dtype=np.float64).reshape(X.shape)


def phi_table(obstacles, X, u):
    """phi[o, i]"""
    x = positions(X, u)
    return np.array([[phi_grad_hess(ob, xi)[0] for xi in x] for ob in obstacles]).reshape(len(obstacles), len(x))


def gap(obstacles, X, u):
    return phi_table(obstacles, X, u).min(axis=0)


def energy(obstacles, X, u, w=None):
    x = positions(X, u)
    w = np.ones(len(x)) if w is None else np.asarray(w, dtype=np.float64)
    e = 0.0
    for ob in obstacles:
        for i, xi in enumerate(x):
            phi = phi_grad_hess(ob, xi)[0]
            if phi < 0.0:
                e += 0.5 * ob[3] * w[i] * phi * phi
    return e


def force(obstacles, X, u, w=None):
    x = positions(X, u)
    w = np.ones(len(x)) if w is None else np.asarray(w, dtype=np.float64)
    g = np.zeros_like(x)
    for ob in obstacles:
        for i, xi in enumerate(x):
            phi, n, _ = phi_grad_hess(ob, xi)
            if phi < 0.0 and n is not None:
                g[i] += ob[3] * w[i] * phi * n
    return g.reshape(-1)


def blocks(obstacles, X, u, w=None, exact=False):
    """B[i] (d x d) per node"""
    x = positions(X, u)
    d = x.shape[1]
    w = np.ones(len(x)) if w is None else np.asarray(w, dtype=np.float64)
    B = np.zeros((len(x), d, d))
    for ob in obstacles:
        for i, xi in enumerate(x):
            phi, n, H = phi_grad_hess(ob, xi)
            if phi < 0.0 and n is not None:
                curv = phi * H
                B[i] += ob[3] * w[i] * (np.outer(n, n) + (curv if exact else _psd_part(curv)))
    return B


def tangent(obstacles, X, u, w=None, exact=False):
    """the block-diagonal matrix of `blocks`, sparse"""
    return sp.block_diag(list(blocks(obstacles, X, u, w, exact)), format="csr")


class ContactMixin:
    """adds the contact term of `obstacles` (and node weights) to the residual, energy and tangent a problem class provides as
    _base_residual, _base_energy and _base_tangent"""

    def set_contact(self, obstacles=(), node_weights=None, exact=False):
        self.obstacles, self.node_weights, self.exact = list(obstacles), node_weights, exact
        assert self.s == self.d or not self.obstacles

    def contact_force(self, u):
        return force(self.obstacles, self.vertices, u, self.node_weights)

    def contact_energy(self, u):
        return energy(self.obstacles, self.vertices, u, self.node_weights)

    def elastic_energy(self, u):
        return self._base_energy(u)

    def residual(self, u):
        r = self._base_residual(u)
        return r + self.contact_force(u) if self.obstacles else r

    def energy(self, u):
        e = self._base_energy(u)
        return e + self.contact_energy(u) if self.obstacles else e

    def tangent(self, u):
        K = self._base_tangent(u)
        if not self.obstacles:
            return K
        return (K + tangent(self.obstacles, self.vertices, u, self.node_weights, self.exact)).tocsr()


class ContactProblem(ContactMixin, dr.Problem):
    """dr.Problem (the oracle's residual, energy, tangent and mass) with the contact term"""

    def __init__(self, *args, obstacles=(), node_weights=None, exact=False, **kw):
        dr.Problem.__init__(self, *args, **kw)
        self.set_contact(obstacles, node_weights, exact)

    def _base_residual(self, u):
        return dr.Problem.residual(self, u)

    def _base_energy(self, u):
        return dr.Problem.energy(self, u)

    def _base_tangent(self, u):
        return dr.Problem.tangent(self, u)
