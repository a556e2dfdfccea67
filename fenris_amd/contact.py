"""Penalty contact with rigid, fixed obstacles (fh_set_obstacles and the fh_contact_* terms of include/fenris_hip.h).

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

`with_obstacles` on MatrixFreeTangent, MatrixFreeShiftedTangent, MatrixFreeNewton, the time integrators and MatrixFreeEigensolver makes
the obstacles belong to that object: they are handed to the engine before every use, as its Dirichlet nodes are.  An object that was never
given obstacles does not inherit those of another object: it clears them from the engine before its use (the owner hands them over again
at its next use); obstacles set directly with Engine.set_obstacles belong to no object and stay.  MatrixFreeOperator's own map (the
operator, not the tangent), the assemblers and the recovery do not include the term; Contact gives its pieces to users of the assembled
path.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi

OBSTACLE_HALF_SPACE, OBSTACLE_BALL, OBSTACLE_CAVITY = 0, 1, 2
MAX_OBSTACLES = 16


def _vec3(v, name):
    a = np.asarray(v, dtype=np.float64).ravel()
    if a.size not in (2, 3):
        raise ValueError(f"{name} must have 2 or 3 components")
    out = np.zeros(3)
    out[:a.size] = a
    return out


class _Obstacle:
    kind = -1

    def __init__(self, point, normal, radius, stiffness, friction=0.0):
        self.point, self.normal = _vec3(point, "point"), _vec3(normal, "normal")
        self.radius, self.stiffness, self.friction = float(radius), float(stiffness), float(friction)

    def _fill(self, o):
        o.kind, o.stiffness, o.radius = self.kind, self.stiffness, self.radius
        for a in range(3):
            o.point[a], o.normal[a] = self.point[a], self.normal[a]


class HalfSpace(_Obstacle):
    """phi(x) = (x - point) . n with n = normal / |normal| (fenris-geometry primitives/half_space.rs): the body stays where phi > 0"""
    kind = OBSTACLE_HALF_SPACE

    def __init__(self, point, normal, stiffness, friction=0.0):
        super().__init__(point, normal, 0.0, stiffness, friction)


class Ball(_Obstacle):
    """phi(x) = |x - centre| - radius (sdf.rs circle, primitives/ball.rs): the body stays outside"""
    kind = OBSTACLE_BALL

    def __init__(self, centre, radius, stiffness, friction=0.0):
        super().__init__(centre, (0.0, 0.0, 0.0), radius, stiffness, friction)


class Cavity(_Obstacle):
    """phi(x) = radius - |x - centre|: the body stays inside"""
    kind = OBSTACLE_CAVITY

    def __init__(self, centre, radius, stiffness, friction=0.0):
        super().__init__(centre, (0.0, 0.0, 0.0), radius, stiffness, friction)


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
        item._fill(o)
    w = obstacles.node_weights
    if w is not None and n and w.size != engine.num_nodes():
        raise ValueError(f"node_weights must hold {engine.num_nodes()} entries")
    engine._check(engine._lib.fh_set_obstacles(engine._h, arr, n, _ffi.fp(w) if (w is not None and n) else None))
    if eps is not None:
        mu = np.array([getattr(o, "friction", 0.0) for o in obstacles.obstacles], dtype=np.float64)
        engine._check(engine._lib.fh_set_friction(engine._h, _ffi.fp(mu), n, eps))


def bind_obstacles(obj, force=False):
    """the `_bind` step of the matrix-free objects: hand the object's obstacles to its engine unless it used the engine last"""
    if not getattr(obj, "_owns_obstacles", False):
        if getattr(obj.engine, "_contact_bound", None) is not None:   # another object's obstacles: not this one's to solve with
            set_obstacles(obj.engine, None)
        return
    if force or getattr(obj.engine, "_contact_bound", None) is not obj:
        set_obstacles(obj.engine, obj._obstacles, getattr(obj, "dt", None))
        obj.engine._contact_bound = obj
        _send_friction_reference(obj)


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
    bind_obstacles(obj, force=True)
    return obj


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

    def gap(self, device=False):
        """per node the smallest phi over the obstacles (negative: penetration)"""
        import torch

        g = torch.empty(self.engine.num_nodes(), dtype=torch.float64, device=f"cuda:{self.engine.device}")
        self.engine._check(self.engine._lib.fh_contact_gap_dev(self.engine._h, C.c_void_p(g.data_ptr())))
        return g if device else g.cpu().numpy()

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
