"""NumPy statement of the sampled signed-distance obstacle FH_OBSTACLE_GRID (include/fenris_hip.h), for tests/test_sdf_grid.py, on top of
contact_reference.py, friction_reference.py and motion_reference.py (all imported unchanged).

A grid obstacle is a tuple ("grid", origin, (values, spacing), k): `values` of shape (nx, ny[, nz]) indexed [ix, iy, iz], `spacing` one h per
axis, sample (0, ..) at `origin`.  With t_a = (x_a - origin_a) / h_a a point is inside iff 0 <= t_a <= n_a - 1 on every axis (a NaN is
outside); i_a = min(floor(t_a), n_a - 2), f_a = t_a - i_a; phi is the bi- / trilinear interpolant of the corner samples of cell i at f,
m its gradient in x (not a unit vector) and Hess phi its second derivative (zero diagonal).  Outside the obstacle does not exist:
phi = +inf, no gradient.  Inside, with p = min(0, phi):
    E = (k w / 2) p^2,   g = k w p m,   B = k w [phi < 0] (m m^T + p Hess phi)  (exact)   or   k w [phi < 0] m m^T  (what the library applies)
and in friction nbar = m / |m|, lam = k w max(0, -phi) |m| at the lag position.  A flat spot (|m| == 0) counts in E and gives nothing else.

The other three kinds go to contact_reference.  So that ContactMixin, friction_reference and motion_reference work on lists that hold
grids, importing this module puts a dispatcher in front of contact_reference.phi_grad_hess and friction_reference._eval: a "grid" tuple is
answered here, every other tuple by the function that stood there, unchanged.

Two analytic twins: linear_field (reproduced exactly: a grid of it is the half-space wherever the box reaches) and curved_field
(phi = z - z0 - c (x - x0)(y - y0) in 3-D, y - y0 - c (x - x0)(y - y0) in 2-D: in the bi- / trilinear space, so reproduced exactly and
globally, with |grad phi| != 1 and no kinks); closed_form evaluates it without a grid, and a tuple ("curved", x0, c, k) is that obstacle in
closed form, everywhere: the reference of the tests that hand the device a grid of it."""
import itertools

import numpy as np
import scipy.sparse as sp

import contact_reference as cr
import friction_reference as fr


def interpolate(values, spacing, origin, x):
    """(inside, phi, m, Hess, cell, f) at one point x"""
    values = np.asarray(values, dtype=np.float64)
    d = values.ndim
    n = np.array(values.shape)
    h = np.asarray(spacing, dtype=np.float64)[:d]
    o = np.asarray(origin, dtype=np.float64)[:d]
    x = np.asarray(x, dtype=np.float64)[:d]
    t = (x - o) / h
    if not np.all((t >= 0.0) & (t <= n - 1)):   # (a NaN compares false: outside)
        return False, np.inf, None, None, None, None
    i = np.minimum(np.floor(t).astype(np.int64), n - 2)
    f = t - i
    W0 = np.stack([1.0 - f, f], axis=1)              # [axis][bit]
    W1 = np.stack([-np.ones(d), np.ones(d)], axis=1)
    phi, m, H = 0.0, np.zeros(d), np.zeros((d, d))
    for bits in itertools.product((0, 1), repeat=d):
        v = values[tuple(i + np.array(bits))]
        phi += v * np.prod([W0[a, bits[a]] for a in range(d)])
        for a in range(d):
            m[a] += v * W1[a, bits[a]] * np.prod([W0[b, bits[b]] for b in range(d) if b != a])
            for b in range(d):
                if b != a:
                    H[a, b] += v * W1[a, bits[a]] * W1[b, bits[b]] * np.prod([W0[c, bits[c]] for c in range(d) if c not in (a, b)])
    return True, float(phi), m / h, H / np.outer(h, h), i, f


SAMPLED = ("grid", "curved")


def _grid_phi_grad_hess(ob, x):
    if ob[0] == "curved":   # twin (b) in closed form: ("curved", x0, c, k), everywhere
        phi, m, H = closed_form(ob[1], ob[2], x)
        return float(phi), m, H
    _, origin, (values, spacing), _ = ob
    inside, phi, m, H, _, _ = interpolate(values, spacing, origin, x)
    if not inside or not np.sqrt(m @ m) > 0.0:
        return phi, None, None
    return phi, m, H


_cr_phi_grad_hess, _fr_eval = cr.phi_grad_hess, fr._eval


def phi_grad_hess(ob, x):
    """(phi, m or None, Hess phi or None): a grid here (m NOT normalised), the other kinds in contact_reference"""
    return _grid_phi_grad_hess(ob, x) if ob[0] in SAMPLED else _cr_phi_grad_hess(ob, x)


def _eval(ob, x, dtype):
    """friction_reference's (phi, nbar): its visit forms lam = k w (-phi), so a grid answers (phi |m|, m / |m|)"""
    if ob[0] not in SAMPLED:
        return _fr_eval(ob, x, dtype)
    phi, m, _ = _grid_phi_grad_hess(ob, np.asarray(x, dtype=np.float64))
    if m is None:
        return dtype(phi), None
    gn = np.sqrt(m @ m)
    return dtype(phi * gn), (m / gn).astype(dtype)


cr.phi_grad_hess, fr._eval = phi_grad_hess, _eval

phi_table, gap, energy, force, positions = cr.phi_table, cr.gap, cr.energy, cr.force, cr.positions   # (through the dispatcher)


def blocks(obstacles, X, u, w=None, exact=False):
    """B[i]: a grid's curvature term is kept (exact) or dropped whole (what the library applies); the other kinds as contact_reference"""
    x = positions(X, u)
    d = x.shape[1]
    w = np.ones(len(x)) if w is None else np.asarray(w, dtype=np.float64)
    B = cr.blocks([ob for ob in obstacles if ob[0] not in SAMPLED], X, u, w, exact)
    for ob in obstacles:
        if ob[0] not in SAMPLED:
            continue
        for i, xi in enumerate(x):
            phi, m, H = phi_grad_hess(ob, xi)
            if phi < 0.0 and m is not None:
                B[i] += ob[3] * w[i] * (np.outer(m, m) + (phi * H if exact else 0.0))
    return B


def tangent(obstacles, X, u, w=None, exact=False):
    return sp.block_diag(list(blocks(obstacles, X, u, w, exact)), format="csr")


class GridContactProblem(cr.ContactProblem):
    """contact_reference.ContactProblem whose tangent takes the blocks of this module"""

    def tangent(self, u):
        K = self._base_tangent(u)
        if not self.obstacles:
            return K
        return (K + tangent(self.obstacles, self.vertices, u, self.node_weights, self.exact)).tocsr()


def cell_clearance(obstacles, X, u):
    """per grid obstacle: (inside mask, the smallest distance of an inside node to a cell face, in cell units)"""
    out = []
    for ob in obstacles:
        if ob[0] != "grid":
            continue
        inside, clear = [], np.inf
        for xi in positions(X, u):
            ok, _, _, _, _, f = interpolate(ob[2][0], ob[2][1], ob[1], xi)
            inside.append(ok)
            if ok:
                clear = min(clear, float(np.minimum(f, 1.0 - f).min()))
        out.append((np.array(inside), clear))
    return out


# ---- the analytic twins
def sample(f, origin, spacing, shape):
    """values[ix, iy(, iz)] = f at origin + i * spacing"""
    axes = [origin[a] + spacing[a] * np.arange(shape[a]) for a in range(len(shape))]
    pts = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1)
    return np.apply_along_axis(f, -1, pts)


def linear_field(p0, nu):
    p0, nu = np.asarray(p0, dtype=np.float64), np.asarray(nu, dtype=np.float64)
    return lambda x: float((np.asarray(x) - p0) @ nu)


def curved_field(x0, c):
    """3-D: z - z0 - c (x - x0)(y - y0) with x0 = (x0, y0, z0); 2-D: y - y0 - c (x - x0)(y - y0) with x0 = (x0, y0)"""
    x0 = np.asarray(x0, dtype=np.float64)

    def f(x):
        if len(x) == 3:
            return float(x[2] - x0[2] - c * (x[0] - x0[0]) * (x[1] - x0[1]))
        return float(x[1] - x0[1] - c * (x[0] - x0[0]) * (x[1] - x0[1]))

    return f


def closed_form(x0, c, x):
    """(phi, m, Hess) of curved_field at x"""
    x, x0 = np.asarray(x, dtype=np.float64), np.asarray(x0, dtype=np.float64)[:len(x)]
    if len(x) == 3:
        a, b = x[0] - x0[0], x[1] - x0[1]
        H = np.zeros((3, 3))
        H[0, 1] = H[1, 0] = -c
        return x[2] - x0[2] - c * a * b, np.array([-c * b, -c * a, 1.0]), H
    a, b = x[0] - x0[0], x[1] - x0[1]
    H = np.zeros((2, 2))
    H[0, 1] = H[1, 0] = -c
    return x[1] - x0[1] - c * a * b, np.array([-c * b, 1.0 - c * a]), H
