"""NumPy statement of the moving obstacles (fh_set_obstacle_paths, fh_set_obstacle_time), of the prescribed motion of the Dirichlet nodes
(fh_dynamics_set_boundary_motion) and of the force resultants per obstacle (fh_contact_resultants) of include/fenris_hip.h, for
tests/test_moving_obstacles.py and tests/test_boundary_motion.py, on top of contact_reference.py, friction_reference.py and
dynamics_reference.py (all imported unchanged).

Paths.  Obstacle o owns knots (t_k, d_k); its offset d_o(t) is piecewise linear through them -- in a segment, with
w = (t - t_k) / (t_{k+1} - t_k), d = fma(w, d_{k+1} - d_k, d_k) per component, the fma rounded once -- constant before the first knot and
after the last; no knots: zero.  A path is a pair (times, offsets) or None.  The obstacle's point is point_o + d_o(t).

Friction against a moving obstacle.  With c_o = d_o(t) - d_o(t_lag): the solvers and the implicit integrators evaluate nbar, P and lam at
xbar_i against the obstacle at point_o + d_o(t_lag) and take s = P (u_i - ubar_i - c_o); central differences evaluate them at the current
position against the obstacle at point_o + d_o(t) and take s = P (dt v_i - c_o).  The coefficients f0, c1, c2 are friction_reference's.

Integrators.  Step n + 1 sees the clock (t_{n+1}, t_n), t_n = n dt; a_0 sees (t_0, t_0).  With a boundary motion (direction, factor), a
Dirichlet dof holds u_n = fma(g_n - g_0, direction, u_0), g_n = factor[min(n, len - 1)]; central differences give it the half-step velocity
v = ((g_{n+1} - g_n) / dt) direction and a = 0; backward Euler gives it the kinematics of a free dof."""
import math
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

import contact_reference as cr
import dynamics_reference as dr
import friction_reference as fr


def fma(a, b, c):
    """a b + c rounded once: exactly, through rationals"""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def path_offset(path, t):
    """d(t), three components"""
    if path is None or len(path[0]) == 0:
        return np.zeros(3)
    T = np.asarray(path[0], dtype=np.float64)
    O = np.zeros((len(T), 3))
    off = np.asarray(path[1], dtype=np.float64).reshape(len(T), -1)
    O[:, :off.shape[1]] = off
    if t <= T[0]:
        return O[0].copy()
    if t >= T[-1]:
        return O[-1].copy()
    k = max(i for i in range(len(T) - 1) if T[i] <= t)
    w = (t - T[k]) / (T[k + 1] - T[k])
    return np.array([fma(w, O[k + 1, a] - O[k, a], O[k, a]) for a in range(3)])


def placed(obstacles, paths, t):
    """the obstacles at point + d(t)"""
    out = []
    for ob, path in zip(obstacles, paths):
        kind, p, q, k = ob
        d = path_offset(path, t)
        out.append((kind, tuple(float(x) + float(d[a]) for a, x in enumerate(p)), q, k))
    return out


def displacements(paths, t, t_lag):
    """c_o = d_o(t) - d_o(t_lag) per obstacle"""
    return [path_offset(q, t) - path_offset(q, t_lag) for q in paths]


# ---- the friction term with the relative slip: friction_reference's visit, obstacle by obstacle, on the slip d - c_o
def _visit(lag_obstacles, mu, X, ubar, d, c, w, dtype=np.float64):
    """yields (o, node, mu lam, nbar, s, y); lag_obstacles: where nbar and lam are taken (the lag position, or the current one for central
    differences)"""
    X = np.asarray(X)
    dim = X.shape[1]
    d = np.asarray(d, dtype=dtype).reshape(X.shape)
    for o, (ob, m) in enumerate(zip(lag_obstacles, mu)):
        rel = d - np.asarray(c[o], dtype=dtype)[:dim]
        for item in fr._visit([ob], [m], X, ubar, rel, w, dtype):
            yield (o,) + item


def friction_potential(lag_obstacles, mu, X, ubar, d, c, eps, w=None):
    return float(sum(ml * fr._coefficients(y, np.float64(eps))[0] for _, _, ml, _, _, y in _visit(lag_obstacles, mu, X, ubar, d, c, w)))


def friction_force(lag_obstacles, mu, X, ubar, d, c, eps, w=None, only=None):
    q = np.zeros(np.shape(X))
    for o, i, ml, _, s, y in _visit(lag_obstacles, mu, X, ubar, d, c, w):
        if only is None or o == only:
            q[i] += ml * fr._coefficients(y, np.float64(eps))[1] * s
    return q.reshape(-1)


def friction_blocks(lag_obstacles, mu, X, ubar, d, c, eps, w=None):
    N, dim = np.shape(X)
    H = np.zeros((N, dim, dim))
    for _, i, ml, n, s, y in _visit(lag_obstacles, mu, X, ubar, d, c, w):
        _, c1, c2 = fr._coefficients(y, np.float64(eps))
        H[i] += ml * (c1 * (np.eye(dim) - np.outer(n, n)) - c2 * np.outer(s, s))
    return H


def friction_tangent(*args, **kw):
    return sp.block_diag(list(friction_blocks(*args, **kw)), format="csr")


def slips(lag_obstacles, mu, X, ubar, d, c, w=None):
    """every |s| of the active pairs"""
    return [float(y) for _, _, _, _, _, y in _visit(lag_obstacles, mu, X, ubar, d, c, w)]


def resultants(obstacles, X, u, w=None, mu=None, lag_obstacles=None, ubar=None, d=None, c=None, eps=None):
    """(R, Q): per obstacle the column sums of its share of g and of q (zeros without mu), each (count, dim)"""
    dim = np.shape(X)[1]
    R = np.array([cr.force([ob], X, u, w).reshape(-1, dim).sum(axis=0) for ob in obstacles])
    Q = np.zeros_like(R)
    if mu is not None:
        for o in range(len(obstacles)):
            Q[o] = friction_force(lag_obstacles, mu, X, ubar, d, c, eps, w, only=o).reshape(-1, dim).sum(axis=0)
    return R, Q


# ---- the problem with a contact clock
class MovingProblem:
    """wraps a contact problem (cr.ContactMixin): its obstacles follow `paths` with the clock of set_time, friction (mu, may be None)
    takes the relative slip.  residual / tangent: the implicit form, at the lag displacement self.ubar; explicit_force: central differences"""

    def __init__(self, prob, paths, mu=None):
        self.prob, self.paths, self.mu = prob, list(paths), (None if mu is None else list(mu))
        self.base = list(prob.obstacles)
        assert len(self.paths) == len(self.base)
        self.eps = None
        self.ubar = np.zeros(prob.n)
        self.set_time(0.0, 0.0)

    def __getattr__(self, name):
        return getattr(self.prob, name)

    def set_time(self, t, t_lag):
        self.prob.obstacles = placed(self.base, self.paths, t)
        self.lag = placed(self.base, self.paths, t_lag)
        self.c = displacements(self.paths, t, t_lag)

    def friction_force(self, u):
        if self.mu is None:
            return np.zeros(self.prob.n)
        p = self.prob
        return friction_force(self.lag, self.mu, p.vertices, self.ubar, np.asarray(u) - self.ubar, self.c, self.eps, p.node_weights)

    def residual(self, u):
        return self.prob.residual(u) + self.friction_force(u)

    def energy(self, u):
        return self.prob.energy(u)

    def tangent(self, u):
        K = self.prob.tangent(u)
        if self.mu is None:
            return K
        p = self.prob
        return (K + friction_tangent(self.lag, self.mu, p.vertices, self.ubar, np.asarray(u) - self.ubar, self.c, self.eps, p.node_weights)).tocsr()

    def explicit_force(self, u, v, dt):
        """the lag configuration is the current one, the slip dt v - c_o"""
        if self.mu is None:
            return np.zeros(self.prob.n)
        p = self.prob
        return friction_force(p.obstacles, self.mu, p.vertices, u, dt * np.asarray(v), self.c, self.eps, p.node_weights)

    def slips(self, u, v=None, dt=None):
        """the |s| of the active pairs as the scheme sees them (v given: central differences)"""
        if self.mu is None:
            return []
        p = self.prob
        if v is not None:
            return slips(p.obstacles, self.mu, p.vertices, u, dt * np.asarray(v), self.c, p.node_weights)
        return slips(self.lag, self.mu, p.vertices, self.ubar, np.asarray(u) - self.ubar, self.c, p.node_weights)

    def in_contact(self, u):
        """whether some node touches an obstacle that has a path, at the clock's current time"""
        p = self.prob
        moving = [ob for ob, q in zip(p.obstacles, self.paths) if q is not None and len(q[0])]
        return bool(moving) and bool((cr.phi_table(moving, p.vertices, u) < 0.0).any())


class Motion:
    """a boundary motion: u_n = fma(g_n - g_0, direction, u_0) on the Dirichlet dofs"""

    def __init__(self, direction, factor):
        self.direction, self.factor = np.asarray(direction, dtype=np.float64).reshape(-1), np.asarray(factor, dtype=np.float64).reshape(-1)

    def g(self, n):
        return float(self.factor[min(n, len(self.factor) - 1)])

    def u(self, n, u0):
        dg = self.g(n) - self.g(0)
        return np.array([fma(dg, e, x) for e, x in zip(self.direction, u0)])

    def half_velocity(self, n, dt):
        """of the drift from step n to n + 1"""
        return ((self.g(n + 1) - self.g(n)) / dt) * self.direction


def _stiffness_force(mp, u, w, eta_k):
    if eta_k == 0.0:
        return 0.0
    prob = mp.prob if isinstance(mp, MovingProblem) else mp
    T = prob._base_tangent(u) if hasattr(prob, "_base_tangent") else prob.tangent(u)
    return eta_k * np.asarray(T @ w).reshape(-1)


def central_difference(mp, u0, v0, dt, steps, record_every=0, eps_v=None, motion=None, eta_k=0.0, probe=None):
    """(u, v, a, records) after `steps` steps; mp: a MovingProblem (or any problem with explicit_force / set_time); motion: a Motion or
    None; eta_k: stiffness damping on the velocity the handle holds; probe(step, mp, u, v_slip) after every residual"""
    fr_ = mp.free
    m = mp.lumped()
    if eps_v is not None:
        mp.eps = eps_v * dt
    u0 = np.array(u0, dtype=np.float64)
    u = u0.copy()
    v = np.array(v0, dtype=np.float64) if motion is not None else np.where(fr_, v0, 0.0)
    mp.set_time(0.0, 0.0)
    a = np.zeros(mp.n)
    a[fr_] = (mp.lf(0) * mp.f - mp.prob.residual(u) - mp.explicit_force(u, v, dt) - _stiffness_force(mp, u, v, eta_k))[fr_] / m[fr_]
    rows = []
    for j in range(steps):
        vh = np.where(fr_, v + 0.5 * dt * a, 0.0)
        un = u + dt * vh
        if motion is not None:
            vh = np.where(fr_, vh, motion.half_velocity(j, dt))
            un = np.where(fr_, un, motion.u(j + 1, u0))
        u = np.where(fr_, un, un if motion is not None else u)
        mp.set_time((j + 1) * dt, j * dt)
        a = np.zeros(mp.n)
        a[fr_] = (mp.lf(j + 1) * mp.f - mp.prob.residual(u) - mp.explicit_force(u, vh, dt) - _stiffness_force(mp, u, vh, eta_k))[fr_] / m[fr_]
        if probe is not None:
            probe(j + 1, mp, u, vh)
        v = np.where(fr_, vh + 0.5 * dt * a, vh)
        if dr._is_record(j, steps, record_every):
            dr._record(mp, rows, 0.5 * float(np.sum(m[fr_] * v[fr_] ** 2)), u, j + 1, dt)
    return u, v, a, np.array(rows)


def implicit(mp, scheme, u0, v0, dt, steps, record_every=0, eps_v=None, motion=None, beta=0.25, gamma=0.5, tol=1e-8, max_it=60, probe=None):
    """Newmark ("newmark") or backward Euler ("euler"; a Motion only here): (u, v, a, records); asserts that every Newton solve converges"""
    fr_ = mp.free
    M = mp.mass()
    euler = scheme == "euler"
    assert motion is None or euler
    nb = 1.0 if euler else beta
    if eps_v is not None:
        mp.eps = eps_v * dt
    u0 = np.array(u0, dtype=np.float64)
    u = u0.copy()
    v = np.array(v0, dtype=np.float64) if motion is not None else np.where(fr_, v0, 0.0)
    a = np.zeros(mp.n)
    mp.set_time(0.0, 0.0)
    mp.ubar = u.copy()
    if not euler:
        a = mp.solve_free(M, mp.lf(0) * mp.f - mp.residual(u))      # (ubar = u_0, c = 0: no friction force)
    rows = []
    moved = ~fr_ if motion is not None else np.zeros(mp.n, dtype=bool)
    kin = fr_ | moved
    for j in range(steps):
        mp.set_time((j + 1) * dt, j * dt)
        mp.ubar = u.copy()
        load = mp.lf(j + 1) * mp.f
        u_ref = np.where(kin, u + dt * v + (0.0 if euler else dt * dt * (0.5 - beta)) * a, u)
        guess = u_ref.copy()
        if motion is not None:
            guess = np.where(fr_, guess, motion.u(j + 1, u0))

        def F(x):
            out = M @ (x - u_ref) + nb * dt * dt * (mp.residual(x) - load)
            out[~fr_] = 0.0
            return out

        def J(x):
            return (M + nb * dt * dt * mp.tangent(x)).tocsr()

        status, un, _ = dr.newton(mp, F, J, guess, tol, True, max_it)
        assert status == "ok", (status, j)
        if probe is not None:
            probe(j + 1, mp, un, None)
        if euler:
            vn = np.where(kin, (un - u) / dt, 0.0)
            a = np.where(kin, (vn - v) / dt, 0.0)
            v = vn
        else:
            an = np.where(fr_, (un - u_ref) / (beta * dt * dt), 0.0)
            v = np.where(fr_, v + dt * ((1.0 - gamma) * a + gamma * an), 0.0)
            a = an
        u = un
        if dr._is_record(j, steps, record_every):
            dr._record(mp, rows, 0.5 * float(v @ (M @ v)), u, j + 1, dt)
    return u, v, a, np.array(rows)


class Still:
    """a problem without obstacles behind MovingProblem's interface, for the runs with a boundary motion alone"""

    def __init__(self, prob):
        self.prob, self.eps, self.ubar = prob, None, None

    def __getattr__(self, name):
        return getattr(self.prob, name)

    def set_time(self, t, t_lag):
        pass

    def explicit_force(self, u, v, dt):
        return 0.0

    def residual(self, u):
        return self.prob.residual(u)

    def tangent(self, u):
        return self.prob.tangent(u)


# ---- the tolerance, measured from the reference alone (the method of tests/test_damping.py::_measured_tolerance)
def rel_diff(x, y):
    """the largest difference over (u, v, a, every record column), each relative to the first trajectory's largest magnitude"""
    out = 0.0
    for p, q in zip(x[:3], y[:3]):
        out = max(out, np.abs(p - q).max() / max(np.abs(p).max(), 1e-300))
    for col in range(4):
        out = max(out, np.abs(x[3][:, col] - y[3][:, col]).max() / max(np.abs(x[3][:, col]).max(), 1e-300))
    return out


def measured_tolerance(run, newton_tol=0.0):
    """run(perm, tol) -> (u, v, a, records) of the reference; perm None or a seed that permutes the connectivity.  d_perm from a permuted
    connectivity, d_newton (newton_tol > 0: an implicit scheme) from a Newton tolerance 100 times smaller; the tolerance is
    20 (d_perm + d_newton), never below 1e-13.  Returns (ref, d_perm, d_newton, tolerance)"""
    ref = run(None, newton_tol)
    d_perm = rel_diff(ref, run(7, newton_tol))
    d_newton = rel_diff(ref, run(None, newton_tol / 100.0)) if newton_tol > 0.0 else 0.0
    return ref, d_perm, d_newton, max(20.0 * (d_perm + d_newton), 1e-13)


def shifted_back(current_obstacles, c):
    """the lag obstacles the other way round: (point + d(t)) - c_o instead of point + d(t_lag); equal up to one rounding of the point"""
    return [(kind, tuple(float(x) - float(co[a]) for a, x in enumerate(p)), q, k) for (kind, p, q, k), co in zip(current_obstacles, c)]


def measured_term_tolerance(run):
    """the same method for a node term (force, potential, blocks, resultants): run(perm) -> a list of arrays of the reference.  The term
    reads no connectivity and solves nothing, so a permuted connectivity changes no bit and there is no d_newton; the one freedom the
    reference has is where it takes the lag obstacle from, and perm selects it: None places it at point + d(t_lag), anything else shifts
    the current point back by c_o (shifted_back).  d_perm is the largest relative difference of the two, piece by piece; the tolerance is
    20 d_perm, never below 1e-13.  Returns (ref, d_perm, 0.0, tolerance)"""
    ref, other = run(None), run(7)
    d_perm = max(np.abs(np.asarray(p) - np.asarray(q)).max() / max(np.abs(np.asarray(p)).max(), 1e-300) for p, q in zip(ref, other))
    return ref, d_perm, 0.0, max(20.0 * d_perm, 1e-13)


def check_constants(table, key, d_perm, d_newton, tol):
    """the measured constants stay within a factor 10 of the table's; returns the table's tolerance"""
    c_perm, c_newton, c_tol = table[key]
    print(f"{key}: d_perm {d_perm:.3e} (constant {c_perm:.3e}), d_newton {d_newton:.3e} ({c_newton:.3e}), tolerance {tol:.3e} ({c_tol:.3e})")
    assert c_tol / 10.0 <= tol <= 10.0 * c_tol, (key, d_perm, d_newton, tol)
    return c_tol


def assert_parity(got, ref, tol, what=""):
    worst = 0.0
    for name, p, q in zip("uva", got[:3], ref[:3]):
        err = np.abs(p - q).max() / max(np.abs(q).max(), 1e-300)
        print(f"{what} {name}: {err:.3e} (tol {tol:.3e})")
        worst = max(worst, err)
    for col, name in enumerate(("kinetic", "stored", "load_potential", "time")):
        err = np.abs(got[3][:, col] - ref[3][:, col]).max() / max(np.abs(ref[3][:, col]).max(), 1e-300)
        print(f"{what} {name}: {err:.3e} (tol {tol:.3e})")
        worst = max(worst, err)
    assert worst <= tol, (what, worst, tol)


def galilean_check(d=3, seed=3):
    """the reference's own Galilean check: shifting every node's slip and the obstacle's displacement by the same vector changes neither
    the friction force nor the potential; and a node that moves with the obstacle (d_i = c_o) has s = 0, q = 0 and f0 = eps / 3.  Returns
    the largest relative difference of the first statement"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (40, d))
    obs = [("half_space", (0.3,) * d, (1.0, 2.0, 3.0)[:d], 1.0e4), ("ball", (1.1,) * d, 0.7, 2.0e3), ("cavity", (0.4, 0.5, 0.6)[:d], 0.75 if d == 3 else 0.6, 5.0e3)]
    mu, eps = [0.5, 0.3, 0.7], 2.0 ** -7
    ubar = rng.uniform(-0.02, 0.02, X.size)
    slip = rng.uniform(-0.02, 0.02, X.shape) * rng.choice([0.1, 1.0], (len(X), 1))
    c = [np.zeros(3)] * 3
    shift = np.zeros(3)
    shift[:d] = rng.uniform(-0.5, 0.5, d)
    q0, D0 = friction_force(obs, mu, X, ubar, slip, c, eps), friction_potential(obs, mu, X, ubar, slip, c, eps)
    q1 = friction_force(obs, mu, X, ubar, slip + shift[:d], [shift] * 3, eps)
    D1 = friction_potential(obs, mu, X, ubar, slip + shift[:d], [shift] * 3, eps)
    assert np.abs(q0).max() > 0.0
    co = friction_force(obs, mu, X, ubar, np.broadcast_to(shift[:d], X.shape), [shift] * 3, eps)
    lam = sum(ml for _, _, ml, _, _, _ in _visit(obs, mu, X, ubar, np.zeros(X.shape), c, None))
    assert not co.any()
    assert math.isclose(friction_potential(obs, mu, X, ubar, np.broadcast_to(shift[:d], X.shape), [shift] * 3, eps), lam * eps / 3.0, rel_tol=1e-14)
    return max(np.abs(q1 - q0).max() / np.abs(q0).max(), abs(D1 - D0) / abs(D0))
