"""Penalty contact with rigid obstacles, fixed or translating along a path (fh_set_obstacles and the fh_contact_* terms of include/fenris_hip.h).

    floor = HalfSpace(point=(0, 0, 0), normal=(0, 0, 1), stiffness=1e4)
    newton = MatrixFreeNewton(asm).with_dirichlet_nodes(top).with_obstacles(Obstacles([floor]))
    newton.solve(u)

An obstacle has a signed distance phi(x), positive where the body may be.  With x_i = X_i + u_i, p = min(0, phi(x_i)) and a node weight
w_i (default 1) the term adds the energy sum (k w_i / 2) p^2, the force k w_i p grad phi to the residual and a symmetric positive
semi-definite block per node to the tangent.  HalfSpace and Cavity (the body stays inside the sphere) give the exact tangent; for Ball
(the body stays outside) the curvature term is negative semi-definite and is dropped: a Gauss-Newton tangent.

Coulomb friction (fh_set_friction): an obstacle takes `friction=mu`, the Obstacles a `slip_length` (the solvers) or a `slip_velocity` (the
time integrators, whose slip length is slip_velocity dt).  The law is lagged and smoothed: normal force and tangent plane are frozen at a lag
displacement ubar, where the friction force is the gradient of a convex potential and its block per node symmetric positive semi-definite.
`with_friction_reference(ubar)` on MatrixFreeNewton, MatrixFreeTangent and MatrixFreeShiftedTangent sets ubar (a quasi-static user moves it
to the converged u between load steps); Newmark and BackwardEuler set ubar = u_n at the start of every step, CentralDifference takes the
current position and the slip of the half-step velocity.  The first-order integrators refuse friction.

Moving obstacles (fh_set_obstacle_paths): an obstacle takes `path=ObstaclePath(times, offsets)`, a piecewise-linear translation of its
point in time, constant before the first knot and after the last.  The second-order time integrators drive the contact clock themselves
(step n + 1 sees the obstacle at t_{n+1} and, for friction, its displacement since t_n); a solver's user calls
`Engine.set_obstacle_time(t, t_lag)`.  The slip of the friction term is taken relative to the obstacle: a node that moves with it feels no
friction.  The first-order integrators refuse paths.  `Contact.resultants()` gives the force the body exerts on each obstacle.

Obstacles of any shape (FH_OBSTACLE_GRID): `SdfGrid(values, spacing)` is a signed distance sampled on a regular grid -- from an array, or
`SdfGrid.from_function(sdf_union(sdf_circle(c, r), sdf_box(lo, hi)), lower, upper, shape)` -- and `GridObstacle(grid, origin, stiffness,
friction=, path=)` the obstacle it makes with its first sample at `origin`.  The device interpolates it bi- / trilinearly; grad phi need
not be a unit vector (force k w p grad phi, Gauss-Newton block k w grad phi grad phi^T).  Outside the box of the samples the obstacle does
not exist: the box must cover every place a node can be while phi < 0.  The samples are uploaded once per (engine, grid).

Augmented Lagrangian (fh_set_contact_multipliers, fh_contact_multiplier_update): a multiplier per obstacle and node, kept as a length
s_oi >= 0 that stands for the force k_o w_i s_oi.  The term is then formed from phi_eff = phi - s_oi wherever it was formed from phi, and
the update s <- max(0, s - phi) between solves drives the penetration to zero at a fixed, moderate k:

    newton = MatrixFreeNewton(asm).with_load(f).with_obstacles(Obstacles([floor]))
    result = AugmentedLagrangian(newton, tol=1e-10).solve(u, NewtonSettings(30, 1e-11))

`Contact.multipliers()`, `.set_multipliers(s)`, `.multiplier_forces()` and `.update_multipliers()` are the pieces.  Every solver and
integrator sees the multipliers as a frozen field; they are kept with the object whose obstacles are bound and travel with them.

`with_obstacles` on MatrixFreeTangent, MatrixFreeShiftedTangent, MatrixFreeNewton, the time integrators and MatrixFreeEigensolver makes
the obstacles belong to that object: they are handed to the engine before every use, as its Dirichlet nodes are.  An object that was never
given obstacles does not inherit those of another object: it clears them from the engine before its use (the owner hands them over again
at its next use); obstacles set directly with Engine.set_obstacles belong to no object and stay.  MatrixFreeOperator's own map (the
operator, not the tangent), the assemblers and the recovery do not include the term; Contact gives its pieces to users of the assembled
path.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _ffi

OBSTACLE_HALF_SPACE, OBSTACLE_BALL, OBSTACLE_CAVITY, OBSTACLE_GRID = 0, 1, 2, 3
MAX_OBSTACLES = 16
MAX_SDF_GRIDS = 16


def _vec3(v, name):
    a = np.asarray(v, dtype=np.float64).ravel()
    if a.size not in (2, 3):
        raise ValueError(f"{name} must have 2 or 3 components")
    out = np.zeros(3)
    out[:a.size] = a
    return out


class ObstaclePath:
    """The translation d(t) of an obstacle: piecewise linear through the knots (times[k], offsets[k]), times strictly increasing, constant
    before the first knot and after the last.  `offset(t)` is fh_set_obstacle_paths' formula in pure Python: in a segment, with
    w = (t - t_k) / (t_{k+1} - t_k), d = fma(w, d_{k+1} - d_k, d_k) per component"""

    def __init__(self, times, offsets):
        self.times = np.ascontiguousarray(np.asarray(times, dtype=np.float64).ravel()).copy()
        off = np.asarray(offsets, dtype=np.float64)
        off = off.reshape(len(self.times), -1) if off.size else off.reshape(0, 3)
        if off.shape[1] not in (2, 3):
            raise ValueError("offsets must have 2 or 3 components per knot")
        self.offsets = np.zeros((len(self.times), 3))
        self.offsets[:, :off.shape[1]] = off
        if not (np.all(np.isfinite(self.times)) and np.all(np.isfinite(self.offsets))):
            raise ValueError("the knots of a path must be finite")
        if np.any(np.diff(self.times) <= 0.0):
            raise ValueError("the knot times of a path must be strictly increasing")

    @classmethod
    def constant_velocity(cls, velocity, t_end):
        """from rest at the origin at t = 0 to velocity * t_end at t_end"""
        v = _vec3(velocity, "velocity")
        return cls([0.0, float(t_end)], [np.zeros(3), v * float(t_end)])

    def __len__(self):
        return len(self.times)

    def offset(self, t):
        T, O = self.times, self.offsets
        if len(T) == 0:
            return np.zeros(3)
        t = float(t)
        if not t > T[0]:
            return O[0].copy()
        if not t < T[-1]:
            return O[-1].copy()
        k = int(np.searchsorted(T, t, side="right")) - 1   # T[k] <= t < T[k + 1]
        w = (t - T[k]) / (T[k + 1] - T[k])
        return np.array([_fma(w, O[k + 1, a] - O[k, a], O[k, a]) for a in range(3)])


def _fma(a, b, c):
    """a b + c rounded once (math.fma where Python has it; else exactly, through rationals)"""
    import math

    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    from fractions import Fraction

    return float(Fraction(a) * Fraction(b) + Fraction(c))


class _Obstacle:
    kind = -1

    def __init__(self, point, normal, radius, stiffness, friction=0.0, path=None):
        self.point, self.normal = _vec3(point, "point"), _vec3(normal, "normal")
        self.radius, self.stiffness, self.friction = float(radius), float(stiffness), float(friction)
        if path is not None and not isinstance(path, ObstaclePath):
            raise TypeError("path must be an ObstaclePath")
        self.path = path

    def _fill(self, o, engine=None):
        o.kind, o.stiffness, o.radius = self.kind, self.stiffness, self.radius
        for a in range(3):
            o.point[a], o.normal[a] = self.point[a], self.normal[a]


class HalfSpace(_Obstacle):
    """phi(x) = (x - point) . n with n = normal / |normal| (fenris-geometry primitives/half_space.rs): the body stays where phi > 0"""
    kind = OBSTACLE_HALF_SPACE

    def __init__(self, point, normal, stiffness, friction=0.0, path=None):
        super().__init__(point, normal, 0.0, stiffness, friction, path)


class Ball(_Obstacle):
    """phi(x) = |x - centre| - radius (sdf.rs circle, primitives/ball.rs): the body stays outside"""
    kind = OBSTACLE_BALL

    def __init__(self, centre, radius, stiffness, friction=0.0, path=None):
        super().__init__(centre, (0.0, 0.0, 0.0), radius, stiffness, friction, path)


class Cavity(_Obstacle):
    """phi(x) = radius - |x - centre|: the body stays inside"""
    kind = OBSTACLE_CAVITY

    def __init__(self, centre, radius, stiffness, friction=0.0, path=None):
        super().__init__(centre, (0.0, 0.0, 0.0), radius, stiffness, friction, path)


class SdfGrid:
    """A signed distance sampled on a regular grid (fh_sdf_grid_create): `values` of shape (nx, ny) or (nx, ny, nz) in numpy's natural
    [ix, iy, iz] index order, `spacing` one h > 0 per axis.  Sample (ix, iy, iz) stands at origin + (ix h_x, iy h_y, iz h_z); the origin
    belongs to the obstacle (GridObstacle), so one grid can stand in several places.  Between the samples phi is the bi- / trilinear
    interpolant; outside their box the obstacle does not exist.  The samples are uploaded lazily, once per (engine, grid)."""

    def __init__(self, values, spacing):
        v = np.asarray(values, dtype=np.float64)
        if v.ndim not in (2, 3):
            raise ValueError("values must have shape (nx, ny) or (nx, ny, nz)")
        h = np.asarray(spacing, dtype=np.float64).ravel()
        if h.size != v.ndim:
            raise ValueError("spacing must have one entry per axis")
        if min(v.shape) < 2:
            raise ValueError("every axis needs at least 2 samples")
        if not (np.all(np.isfinite(h)) and np.all(h > 0.0)):
            raise ValueError("the spacings must be positive and finite")
        if not np.all(np.isfinite(v)):
            raise ValueError("the samples must be finite")
        self.values, self.spacing, self.dim = v.copy(), h.copy(), v.ndim

    @property
    def shape(self):
        return self.values.shape

    @classmethod
    def from_function(cls, f, lower, upper, shape):
        """(grid, origin): the vectorised f(points (m, dim)) -> phi (m) sampled at shape[a] >= 2 equidistant positions per axis from lower
        to upper (both included); origin = lower"""
        lower, upper = np.asarray(lower, dtype=np.float64).ravel(), np.asarray(upper, dtype=np.float64).ravel()
        shape = tuple(int(s) for s in shape)
        if not (lower.size == upper.size == len(shape)) or len(shape) not in (2, 3):
            raise ValueError("lower, upper and shape must have 2 or 3 entries each")
        h = (upper - lower) / (np.array(shape) - 1)
        axes = [lower[a] + h[a] * np.arange(shape[a]) for a in range(len(shape))]
        pts = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, len(shape))
        phi = np.asarray(f(pts), dtype=np.float64).reshape(shape)
        return cls(phi, h), lower.copy()

    def abi_values(self):
        """the samples in the ABI's layout: x fastest"""
        return np.ascontiguousarray(self.values.transpose(tuple(range(self.dim))[::-1])).ravel()

    def evaluate(self, points, origin):
        """(phi, grad) at points (m, dim) with sample (0, ..) at `origin`, on the host, as the device evaluates it: t = (x - origin) / h;
        inside iff 0 <= t_a <= n_a - 1 on every axis (a NaN is outside: phi = +inf, grad = 0); i = min(floor(t), n - 2), f = t - i; phi the
        bi- / trilinear interpolant of the corner samples of cell i at f, grad its gradient in x"""
        d, n, h = self.dim, np.array(self.values.shape), self.spacing
        x = np.asarray(points, dtype=np.float64).reshape(-1, d)
        o = np.asarray(origin, dtype=np.float64).ravel()[:d]
        with np.errstate(invalid="ignore"):
            t = (x - o) / h
            inside = np.all((t >= 0.0) & (t <= (n - 1)), axis=1)
        phi, grad = np.full(len(x), np.inf), np.zeros((len(x), d))
        if not inside.any():
            return phi, grad
        ti = t[inside]
        i = np.minimum(np.floor(ti).astype(np.int64), n - 2)
        f = ti - i
        w = np.stack([1.0 - f, f], axis=-1)   # [point, axis, 0 / 1]
        s, ds = np.zeros(len(ti)), np.zeros((len(ti), d))
        for q in range(1 << d):
            bit = [(q >> a) & 1 for a in range(d)]
            v = self.values[tuple(i[:, a] + bit[a] for a in range(d))]
            prod = v.copy()
            for a in range(d):
                prod = prod * w[:, a, bit[a]]
            s += prod
            for a in range(d):
                part = v if bit[a] else -v
                for b in range(d):
                    if b != a:
                        part = part * w[:, b, bit[b]]
                ds[:, a] += part
        phi[inside] = s
        grad[inside] = ds / h
        return phi, grad

    def _id_on(self, engine):
        """the slot of this grid's upload in `engine` (made at the first use; Engine.close drops the table)"""
        table = engine.__dict__.setdefault("_sdf_grids", {})
        hit = table.get(id(self))
        if hit is not None and hit[0] is self:
            return hit[1]
        n = np.ones(3, dtype=np.uint32)
        n[:self.dim] = self.values.shape
        h = np.ones(3)
        h[:self.dim] = self.spacing
        vals = self.abi_values()
        slot = C.c_uint32(0)
        engine._check(engine._lib.fh_sdf_grid_create(engine._h, self.dim, n.ctypes.data_as(_ffi.u32p), _ffi.fp(h), _ffi.fp(vals), C.byref(slot)))
        table[id(self)] = (self, int(slot.value))   # (the grid is kept alive with its slot: an id() is never reused under it)
        return int(slot.value)


class GridObstacle(_Obstacle):
    """phi(x) = the interpolant of `grid` with its sample (0, ..) at `origin` (FH_OBSTACLE_GRID): any rigid shape.  The body stays where
    phi > 0; outside the box of the samples the obstacle does not exist, so the box must cover every place a node can be while phi < 0.
    grad phi need not be a unit vector: the force is k w p grad phi, the block k w grad phi grad phi^T (Gauss-Newton)"""
    kind = OBSTACLE_GRID

    def __init__(self, grid, origin, stiffness, friction=0.0, path=None):
        if not isinstance(grid, SdfGrid):
            raise TypeError("grid must be an SdfGrid")
        if np.asarray(origin).size != grid.dim:
            raise ValueError("origin must have one entry per axis of the grid")
        super().__init__(origin, (0.0, 0.0, 0.0), 0.0, stiffness, friction, path)
        self.grid = grid

    def _fill(self, o, engine=None):
        if engine is None:
            raise ValueError("a GridObstacle is filled for an engine (its grid is uploaded there)")
        super()._fill(o, engine)
        o.grid = self.grid._id_on(engine)


def sdf_circle(centre, radius):
    """|x - centre| - radius (sdf.rs SdfCircle; a sphere in 3-D), as a callable for SdfGrid.from_function"""
    c, r = np.asarray(centre, dtype=np.float64).ravel(), float(radius)
    return lambda x: np.linalg.norm(np.asarray(x, dtype=np.float64) - c, axis=-1) - r


def sdf_box(lower, upper):
    """the axis-aligned box (sdf.rs SdfAxisAlignedBox): with b the half extents, p = x - centre and d = |p| - b,
    |max(d, 0)| + min(0, max_a d_a)"""
    lo, hi = np.asarray(lower, dtype=np.float64).ravel(), np.asarray(upper, dtype=np.float64).ravel()
    b, mid = (hi - lo) / 2.0, (hi + lo) / 2.0

    def f(x):
        d = np.abs(np.asarray(x, dtype=np.float64) - mid) - b
        return np.linalg.norm(np.maximum(d, 0.0), axis=-1) + np.minimum(0.0, d.max(axis=-1))

    return f


def sdf_union(a, b):
    """min(a, b) (sdf.rs SdfUnion)"""
    return lambda x: np.minimum(a(x), b(x))


class Obstacles:
    """A list of at most MAX_OBSTACLES obstacles and optional node weights w_i >= 0 (one per node; None: 1).  With friction on any of them:
    slip_length (eps of the solvers' term) and / or slip_velocity (the time integrators: eps = slip_velocity dt)"""

    def __init__(self, obstacles, node_weights=None, slip_length=None, slip_velocity=None):
        self.obstacles = list(obstacles)
        self.slip_length = None if slip_length is None else float(slip_length)
        self.slip_velocity = None if slip_velocity is None else float(slip_velocity)
        self.node_weights = None if node_weights is None else np.ascontiguousarray(np.asarray(node_weights, dtype=np.float64).ravel()).copy()

    def __len__(self):
        return len(self.obstacles)

    def has_paths(self):
        return any(getattr(o, "path", None) is not None and len(o.path) for o in self.obstacles)

    def has_friction(self):
        return any(getattr(o, "friction", 0.0) > 0.0 for o in self.obstacles)

    def slip_length_for(self, dt=None):
        """the slip length a user with time step dt (None: a solver) hands to fh_set_friction"""
        if self.slip_length is not None:
            return self.slip_length
        if dt is not None and self.slip_velocity is not None:
            return self.slip_velocity * dt
        raise ValueError("obstacles with friction need a slip_length (solvers) or a slip_velocity (time integrators)")


def set_obstacles(engine, obstacles, dt=None):
    """Engine.set_obstacles: an Obstacles, a plain list of obstacles, or None / empty to clear them.  dt: the time step of the integrator
    that binds them (friction: slip_velocity dt may stand in for the slip length)"""
    engine._contact_bound = None   # (no object's obstacles are bound any more)
    if obstacles is None:
        obstacles = Obstacles([])
    elif not isinstance(obstacles, Obstacles):
        obstacles = Obstacles(obstacles)
    n = len(obstacles)
    eps = obstacles.slip_length_for(dt) if obstacles.has_friction() else None   # (raises before anything is sent)
    arr = (_ffi.Obstacle * max(n, 1))()
    for o, item in zip(arr, obstacles.obstacles):
        item._fill(o, engine)
    w = obstacles.node_weights
    if w is not None and n and w.size != engine.num_nodes():
        raise ValueError(f"node_weights must hold {engine.num_nodes()} entries")
    engine._check(engine._lib.fh_set_obstacles(engine._h, arr, n, _ffi.fp(w) if (w is not None and n) else None))
    if eps is not None:
        mu = np.array([getattr(o, "friction", 0.0) for o in obstacles.obstacles], dtype=np.float64)
        engine._check(engine._lib.fh_set_friction(engine._h, _ffi.fp(mu), n, eps))
    if obstacles.has_paths():   # (after the obstacles, which clear them)
        paths = [getattr(o, "path", None) for o in obstacles.obstacles]
        begin = np.zeros(n + 1, dtype=np.uint64)
        begin[1:] = np.cumsum([0 if q is None else len(q) for q in paths])
        times = np.ascontiguousarray(np.concatenate([q.times for q in paths if q is not None]))
        offsets = np.ascontiguousarray(np.concatenate([q.offsets.ravel() for q in paths if q is not None]))
        engine._check(engine._lib.fh_set_obstacle_paths(engine._h, _ffi.up(begin), _ffi.fp(times), _ffi.fp(offsets)))
    return obstacles


def set_obstacle_time(engine, t, t_lag=None):
    """Engine.set_obstacle_time: the contact clock (fh_set_obstacle_time); t_lag None: t.  The object whose obstacles are bound keeps the
    clock, so that bind_obstacles can send it again with them (the time integrators drive the clock themselves and keep none)"""
    clock = (float(t), float(t if t_lag is None else t_lag))
    engine._check(engine._lib.fh_set_obstacle_time(engine._h, *clock))
    owner = getattr(engine, "_contact_bound", None)
    if owner is not None and getattr(owner, "dt", None) is None:
        owner._contact_clock = clock


def bind_obstacles(obj, force=False):
    """the `_bind` step of the matrix-free objects: hand the object's obstacles to its engine unless it used the engine last.  The contact
    clock Engine.set_obstacle_time gave while they were bound goes with them again (fh_set_obstacles alone returns it to (0, 0))"""
    if not getattr(obj, "_owns_obstacles", False):
        if getattr(obj.engine, "_contact_bound", None) is not None:   # another object's obstacles: not this one's to solve with
            set_obstacles(obj.engine, None)
        return
    if force or getattr(obj.engine, "_contact_bound", None) is not obj:
        clock = getattr(obj, "_contact_clock", None)
        sent = set_obstacles(obj.engine, obj._obstacles, getattr(obj, "dt", None))
        obj.engine._contact_bound = obj
        if clock is not None and len(sent) and sent.has_paths():
            obj.engine._check(obj.engine._lib.fh_set_obstacle_time(obj.engine._h, *clock))
        _send_friction_reference(obj)
        _send_multipliers(obj)


def _send_multipliers(obj):
    """the multipliers kept with the object (a device tensor, count x N) to its engine again: fh_set_obstacles cleared them"""
    s = getattr(obj, "_multipliers", None)
    if s is None or not len(obj._obstacles or ()):
        return
    obj.engine._check(obj.engine._lib.fh_set_contact_multipliers_dev(obj.engine._h, C.c_void_p(s.data_ptr())))


def _has_friction(obj):
    obstacles = getattr(obj, "_obstacles", None)
    return isinstance(obstacles, Obstacles) and obstacles.has_friction()


def _send_friction_reference(obj):
    ref = getattr(obj, "_friction_ref", None)
    if ref is None or not _has_friction(obj):
        return
    eng = obj.engine
    if isinstance(ref, np.ndarray):
        eng._check(eng._lib.fh_set_friction_reference(eng._h, _ffi.fp(ref)))
    else:
        eng._check(eng._lib.fh_set_friction_reference_dev(eng._h, C.c_void_p(ref.data_ptr())))


def with_friction_reference(obj, ubar):
    """the body of `with_friction_reference(ubar)`: the lag displacement of the friction term, a numpy array or device tensor that is COPIED
    here (after a solve: the converged u), so the lag state is what the caller gave whoever uses the engine in between.  It is bound like
    the obstacles; returns obj"""
    if ubar is None:
        raise ValueError("with_friction_reference needs the lag displacement itself (after a solve: the converged u)")
    if isinstance(ubar, np.ndarray) or not hasattr(ubar, "data_ptr"):
        obj._friction_ref = np.ascontiguousarray(np.asarray(ubar, dtype=np.float64).ravel()).copy()
    else:
        obj._friction_ref = ubar.detach().clone().contiguous()
    if getattr(obj, "_owns_obstacles", False):
        bind_obstacles(obj, force=True)
    return obj


def send_slip_velocity(obj):
    """the time integrators: the slip velocity of the object's obstacles to its handle (second-order handles only)"""
    if obj._h is None or not _has_friction(obj) or obj._obstacles.slip_velocity is None or obj._create != "fh_dynamics_create":
        return
    obj.engine._check(obj.engine._lib.fh_dynamics_set_slip_velocity(obj._h, obj._obstacles.slip_velocity))


def with_obstacles(obj, obstacles):
    """the body of `with_obstacles(obstacles)` of those objects (None: none); returns obj"""
    obj._obstacles = obstacles
    obj._owns_obstacles = True
    obj._contact_clock = None   # (new obstacles: the clock starts at (0, 0), as after Engine.set_obstacles)
    obj._multipliers = None     # (and no multipliers stand)
    bind_obstacles(obj, force=True)
    return obj


@dataclass
class MultiplierUpdate:
    """what fh_contact_multiplier_update reports over the counted (node, obstacle) pairs: max_change = max |s_new - s_old| (the convergence
    measure: |phi| where the pair is active afterwards, the released multiplier otherwise), max_penetration = max max(0, -phi), active =
    the number of pairs with s_new > 0, max_force = the largest lam = k w s_new"""

    max_change: float
    max_penetration: float
    active: int
    max_force: float


class Contact:
    """The contact term of an engine's obstacles at its current u, piece by piece, over every node (Dirichlet nodes included): for users
    of the assembled path, who add the force to an assembled residual and the tangent blocks to assembled CSR values."""

    def __init__(self, engine):
        self.engine = getattr(engine, "engine", engine)   # (an element assembler is accepted too)

    def _dim(self):
        return _ffi.ELEM_DIM[self.engine._mesh.elem_kind]

    def energy(self):
        e = C.c_double(0.0)
        self.engine._check(self.engine._lib.fh_contact_energy(self.engine._h, C.byref(e)))
        return e.value

    def force(self, device=False, out=None):
        """g (the force the term adds to r(u)): a new vector, or ADDED into the device tensor `out`"""
        import torch

        if out is None:
            out = torch.zeros(self._dim() * self.engine.num_nodes(), dtype=torch.float64, device=f"cuda:{self.engine.device}")
        self.engine._check(self.engine._lib.fh_contact_force_dev(self.engine._h, C.c_void_p(out.data_ptr())))
        return out if device else out.cpu().numpy()

    def friction_potential(self):
        """D, the potential of the lagged friction term at the engine's u (0 without friction)"""
        e = C.c_double(0.0)
        self.engine._check(self.engine._lib.fh_friction_potential(self.engine._h, C.byref(e)))
        return e.value

    def friction_force(self, device=False, out=None):
        """q (the force the friction term adds to r(u) beside g): a new vector, or ADDED into the device tensor `out`"""
        import torch

        if out is None:
            out = torch.zeros(self._dim() * self.engine.num_nodes(), dtype=torch.float64, device=f"cuda:{self.engine.device}")
        self.engine._check(self.engine._lib.fh_friction_force_dev(self.engine._h, C.c_void_p(out.data_ptr())))
        return out if device else out.cpu().numpy()

    def _count(self):
        """the number of obstacles that stand in the engine (fh_obstacle_count), whoever set them"""
        count = C.c_uint64(0)
        self.engine._check(self.engine._lib.fh_obstacle_count(self.engine._h, C.byref(count)))
        return int(count.value)

    def resultants(self):
        """(normal, friction): per obstacle the share R_o of g -- the force the body exerts on the obstacle -- and the share Q_o of q (zeros
        without friction), each of shape (count, dim), at the engine's u over every node"""
        count = self._count()
        normal, friction = np.zeros(3 * MAX_OBSTACLES), np.zeros(3 * MAX_OBSTACLES)
        self.engine._check(self.engine._lib.fh_contact_resultants(self.engine._h, _ffi.fp(normal), _ffi.fp(friction)))
        d = self._dim()
        return normal[:3 * count].reshape(count, 3)[:, :d].copy(), friction[:3 * count].reshape(count, 3)[:, :d].copy()

    def obstacle_offsets(self):
        """(current, lag): d_o(t) and d_o(t_lag) of the contact clock per obstacle, each of shape (count, dim)"""
        count = self._count()
        cur, lag = np.zeros(3 * MAX_OBSTACLES), np.zeros(3 * MAX_OBSTACLES)
        self.engine._check(self.engine._lib.fh_obstacle_offsets(self.engine._h, _ffi.fp(cur), _ffi.fp(lag)))
        d = self._dim()
        return cur[:3 * count].reshape(count, 3)[:, :d].copy(), lag[:3 * count].reshape(count, 3)[:, :d].copy()

    def gap(self, device=False):
        """per node the smallest phi over the obstacles (negative: penetration)"""
        import torch

        g = torch.empty(self.engine.num_nodes(), dtype=torch.float64, device=f"cuda:{self.engine.device}")
        self.engine._check(self.engine._lib.fh_contact_gap_dev(self.engine._h, C.c_void_p(g.data_ptr())))
        return g if device else g.cpu().numpy()

    def sample_grid(self, grid, origin, points, device=False):
        """(phi, grad) of an SdfGrid with its sample (0, ..) at `origin`, interpolated on the device at points (m, dim): a numpy array or a
        device tensor (fh_sdf_grid_sample_dev); a point outside the box gets +inf and a zero gradient"""
        import torch

        d = grid.dim
        o = np.zeros(3)
        o[:d] = np.asarray(origin, dtype=np.float64).ravel()
        if isinstance(points, torch.Tensor):
            pts = points.to(dtype=torch.float64).contiguous().reshape(-1, d)
        else:
            pts = torch.from_numpy(np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, d))).to(f"cuda:{self.engine.device}")
        m = pts.shape[0]
        phi = torch.empty(m, dtype=torch.float64, device=pts.device)
        grad = torch.empty((m, d), dtype=torch.float64, device=pts.device)
        self.engine._check(self.engine._lib.fh_sdf_grid_sample_dev(self.engine._h, grid._id_on(self.engine), _ffi.fp(o), C.c_void_p(pts.data_ptr()), m,
                                                                   C.c_void_p(phi.data_ptr()), C.c_void_p(grad.data_ptr())))
        return (phi, grad) if device else (phi.cpu().numpy(), grad.cpu().numpy())

    def add_tangent_to(self, csr_values):
        """B (and, while friction is set, H) ADDED into the diagonal node blocks of the engine's CSR values: a device tensor in place, or a numpy array (returned)"""
        import torch

        if isinstance(csr_values, torch.Tensor):
            self.engine._check(self.engine._lib.fh_add_contact_tangent_csr_dev(self.engine._h, C.c_void_p(csr_values.data_ptr())))
            return csr_values
        t = torch.from_numpy(np.ascontiguousarray(csr_values, dtype=np.float64)).to(f"cuda:{self.engine.device}")
        self.engine._check(self.engine._lib.fh_add_contact_tangent_csr_dev(self.engine._h, C.c_void_p(t.data_ptr())))
        csr_values[...] = t.cpu().numpy().reshape(np.shape(csr_values))
        return csr_values

    # ---- augmented Lagrangian: the multipliers, lengths s[o, i] >= 0 that stand for the forces k_o w_i s[o, i]
    def _keep_multipliers(self, standing):
        """the multipliers as they stand now go with the object whose obstacles are bound (bind_obstacles sends them again)"""
        owner = getattr(self.engine, "_contact_bound", None)
        if owner is not None:
            owner._multipliers = self.multipliers(device=True) if standing else None

    def multipliers(self, device=False):
        """s of shape (count, N); zeros while none are set"""
        import torch

        s = torch.empty((self._count(), self.engine.num_nodes()), dtype=torch.float64, device=f"cuda:{self.engine.device}")
        self.engine._check(self.engine._lib.fh_contact_multipliers_dev(self.engine._h, C.c_void_p(s.data_ptr())))
        return s if device else s.cpu().numpy()

    def set_multipliers(self, s):
        """s: (count, N) entries >= 0, a numpy array (checked) or a device tensor (copied as it is); None clears them"""
        eng = self.engine
        if s is None:
            eng._check(eng._lib.fh_set_contact_multipliers(eng._h, None))
        else:
            want = self._count() * eng.num_nodes()
            if hasattr(s, "data_ptr"):
                import torch

                t = s.to(dtype=torch.float64, device=f"cuda:{eng.device}").contiguous()
                if t.numel() != want:
                    raise ValueError(f"the multipliers must hold {want} entries")
                eng._check(eng._lib.fh_set_contact_multipliers_dev(eng._h, C.c_void_p(t.data_ptr())))
            else:
                a = np.ascontiguousarray(np.asarray(s, dtype=np.float64).ravel())
                if a.size != want:
                    raise ValueError(f"the multipliers must hold {want} entries")
                eng._check(eng._lib.fh_set_contact_multipliers(eng._h, _ffi.fp(a)))
        self._keep_multipliers(s is not None)
        return self

    def multiplier_forces(self, device=False):
        """lam of shape (count, N): k_o w_i s[o, i], for a grid times |grad phi| at the node's current position"""
        import torch

        lam = torch.empty((self._count(), self.engine.num_nodes()), dtype=torch.float64, device=f"cuda:{self.engine.device}")
        self.engine._check(self.engine._lib.fh_contact_multiplier_forces_dev(self.engine._h, C.c_void_p(lam.data_ptr())))
        return lam if device else lam.cpu().numpy()

    def update_multipliers(self, skip_nodes=None):
        """s <- max(0, s - phi) at the engine's u (the first call starts from zeros); skip_nodes (the fully held nodes) keep s = 0 and stay
        out of the statistics.  Returns a MultiplierUpdate"""
        skip = np.zeros(0, dtype=np.uint64) if skip_nodes is None else _ffi.as_u64(skip_nodes).reshape(-1)
        st = _ffi.MultiplierUpdateStats()
        self.engine._check(self.engine._lib.fh_contact_multiplier_update(self.engine._h, _ffi.up(skip) if len(skip) else None, len(skip), C.byref(st)))
        self._keep_multipliers(True)
        return MultiplierUpdate(st.max_change, st.max_penetration, int(st.active), st.max_force)


@dataclass
class AugmentedLagrangianResult:
    """updates: the multiplier updates taken; multiplier_updates / newton_results: one entry per update; converged: the last update's
    max_change <= tol"""

    updates: int = 0
    multiplier_updates: list = field(default_factory=list)
    newton_results: list = field(default_factory=list)
    converged: bool = False


class AugmentedLagrangianError(RuntimeError):
    """max_updates multiplier updates without max_change <= tol; `result` holds the partial AugmentedLagrangianResult (u is the last solve's)"""

    def __init__(self, message, result):
        super().__init__(message)
        self.result = result


class AugmentedLagrangian:
    """The Uzawa iteration on a MatrixFreeNewton with obstacles: solve with the multipliers frozen, update them at the solution
    (s <- max(0, s - phi)), and again until the largest change of a multiplier is <= tol.  The penetration goes to zero at the fixed k
    of the obstacles.  The multipliers that stand at entry are the start (a load step warm-starts from the last); the solver's fully held
    Dirichlet nodes keep s = 0."""

    def __init__(self, newton, max_updates=30, tol=1e-10):
        self.newton, self.engine = newton, newton.engine
        self.max_updates, self.tol = int(max_updates), float(tol)

    def with_obstacles(self, obstacles):
        """the obstacles of the underlying solver (its with_obstacles); returns self"""
        self.newton.with_obstacles(obstacles)
        return self

    def _held_nodes(self):
        from .dirichlet import DofSet

        held = DofSet.of(self.newton._nodes)
        full = (1 << self.newton.element_assembler.solution_dim()) - 1
        return held.nodes[(held.masks & full) == full]

    def solve(self, u, settings=None, **newton_kwargs):
        """u: the guess, overwritten by the solution; settings and newton_kwargs go to MatrixFreeNewton.solve.  Returns an
        AugmentedLagrangianResult; raises AugmentedLagrangianError when max_updates run out, and whatever the Newton solve raises"""
        if not getattr(self.newton, "_owns_obstacles", False) or not len(self.newton._obstacles or ()):
            raise ValueError("AugmentedLagrangian needs a solver with obstacles (with_obstacles)")
        result = AugmentedLagrangianResult()
        skip = self._held_nodes()
        con = Contact(self.engine)
        for _ in range(self.max_updates):
            args = () if settings is None else (settings,)
            result.newton_results.append(self.newton.solve(u, *args, **newton_kwargs))   # (binds the obstacles and their multipliers)
            up = con.update_multipliers(skip)
            result.multiplier_updates.append(up)
            result.updates += 1
            if up.max_change <= self.tol:
                result.converged = True
                return result
        raise AugmentedLagrangianError(f"{self.max_updates} multiplier updates, max_change {result.multiplier_updates[-1].max_change:.3e} > {self.tol:.3e}",
                                       result)
