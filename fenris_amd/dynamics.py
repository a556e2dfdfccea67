"""Time integration on the device (fh_dynamics_*, include/fenris_hip.h):  M a + r(u) = lf_n f  with an element assembler's residual and
the mass of MatrixFreeShiftedTangent, by central differences, Newmark(beta, gamma) or backward Euler.

    ti = (CentralDifference(asm, density, dt).with_dirichlet_nodes(clamp).with_load(f, load_factor=np.linspace(0, 1, 8)))
    ti.set_state(u0, v0)
    rec = ti.step(1000, record_every=100)        # rec.kinetic, rec.stored, rec.load_potential, rec.time: one entry per record
    u, v, a, time, step = ti.state()

The whole loop runs in the library: on Hex8, Tet4, Quad4 and Tri3 an explicit step is the residual's element pass and one node pass, and
the host waits only at records.

The first-order problem  M du/dt + r(u) = lf_n f  (heat conduction for the Laplace operator, the gradient flow of the stored energy for the
elastic ones) runs on the same handle (fh_first_order_create): RungeKuttaLegendre (super-stepped explicit; ForwardEuler is its one-stage
case) and ThetaMethod (Crank-Nicolson, implicit Euler).

    ti = RungeKuttaLegendre(asm, capacity, dt, stages=8).with_dirichlet_nodes(cold).with_load(q)
    ti.set_state(u0)
    rec = ti.step(200, record_every=50)          # rec.mass_norm, rec.stored, rec.load_potential, rec.time
    u, rate, time, step = ti.state()

Rayleigh damping  M a + C(u) v + r(u) = lf_n f,  C(u) = eta_m M + eta_k T(u)  (fh_dynamics_set_damping), on the three second-order schemes:

    ti = CentralDifference(asm, density, dt).with_damping(RayleighDamping.from_ratios(0.02, w1, 0.05, w2))
    ti = Newmark(asm, density, dt).with_damping(mass=0.5, stiffness=1e-4)"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _ffi
from . import contact as _contact
from . import dirichlet as _dirichlet
from ._ffi import FenrisError, SingularJacobianError
from .assembly import (BacktrackingLineSearch, JacobianError, LineSearchError, MaximumIterationsReached, NewtonResult, NewtonSettings, _is_torch,
                       _ptr)


class DynamicsError(FenrisError):
    """fh_dynamics_step ended early (FH_DYNAMICS_NONFINITE, or any code that is not a Newton failure); steps_done: the steps of the call
    that stand (for central differences: up to the last clean record)"""

    def __init__(self, code, message, steps_done):
        super().__init__(code, message)
        self.steps_done = steps_done


@dataclass
class DynamicsRecord:
    """the records of one step() call, one entry per record: time, kinetic energy, stored energy, lf f . u; steps_done; stats = (steps,
    residual evaluations, Newton iterations, PCG iterations, records)"""

    time: np.ndarray
    kinetic: np.ndarray
    stored: np.ndarray
    load_potential: np.ndarray
    steps_done: int
    stats: tuple


@dataclass(frozen=True)
class RayleighDamping:
    """C = mass M + stiffness T(u): both coefficients finite and not negative"""

    mass: float = 0.0
    stiffness: float = 0.0

    @classmethod
    def from_ratios(cls, xi1, omega1, xi2, omega2):
        """the coefficients that give the damping ratios xi1 at omega1 and xi2 at omega2 (rad / time), omega1 != omega2: the two-frequency
        fit of xi(omega) = mass / (2 omega) + stiffness omega / 2; a fit with a negative coefficient is refused"""
        xi1, omega1, xi2, omega2 = float(xi1), float(omega1), float(xi2), float(omega2)
        if not (omega1 > 0.0 and omega2 > 0.0 and omega1 != omega2):
            raise ValueError("from_ratios needs two distinct positive frequencies")
        den = (omega2 - omega1) * (omega2 + omega1)
        mass = 2.0 * omega1 * omega2 * (xi1 * omega2 - xi2 * omega1) / den
        stiffness = 2.0 * (xi2 * omega2 - xi1 * omega1) / den
        if mass < 0.0 or stiffness < 0.0:
            raise ValueError(f"these ratios need a negative coefficient (mass {mass}, stiffness {stiffness})")
        return cls(mass, stiffness)

    def ratio(self, omega):
        """the damping ratio of a mode of angular frequency omega"""
        return self.mass / (2.0 * omega) + self.stiffness * omega / 2.0


class TimeIntegrator:
    """The interface the three schemes share.  Density, Dirichlet nodes and load belong to this object and are handed to the engine before
    every use (the discipline of MatrixFreeNewton._bind), so several objects may share one assembler.  The assembler's u is the state's u."""

    scheme = None
    _create = "fh_dynamics_create"

    def __init__(self, element_assembler, density, dt):
        self.element_assembler = element_assembler
        self.engine = element_assembler.engine
        self.dt = float(dt)
        self._rho = np.ascontiguousarray(np.atleast_1d(np.asarray(density, dtype=np.float64)).ravel()).copy()
        self._nodes = None
        self._mg = None
        self._settings = NewtonSettings()
        self._line_search = BacktrackingLineSearch()
        self._linear_rel_tol, self._linear_max_iter = 1e-8, 0
        self._beta, self._gamma = 0.25, 0.5
        self._h = None
        self._load = (None, None)
        self._damping = None
        self._motion = None
        self.engine.set_mass_density(self._rho)   # (checks the count now)
        self.engine._mass_bound = self

    # ---- configuration
    def with_dirichlet_nodes(self, nodes):
        """the nodes held at the u of set_state, with v = a = 0 (None: none); returns self"""
        self._nodes = None if nodes is None else _ffi.as_u64(nodes).copy()
        self._bind(force=True)
        return self

    def with_dirichlet_dofs(self, nodes, components):
        """single components held at the u of set_state with v = a = 0 (MatrixFreeOperator.with_dirichlet_dofs: an (n, S) boolean array
        or component indices); with_boundary_motion moves these components alone; calls accumulate; returns self"""
        return _dirichlet.with_dirichlet_dofs(self, nodes, components)

    def with_load(self, f, load_factor=None):
        """the load f (numpy array or device tensor; None: zero) and the factor per step, lf_n = load_factor[min(n, len - 1)] (None: 1)"""
        self._load = (f, None if load_factor is None else _ffi.as_f64(load_factor).reshape(-1).copy())
        if self._h is not None:
            self._send_load()
        return self

    def with_damping(self, mass=0.0, stiffness=0.0):
        """Rayleigh damping C = mass M + stiffness T(u) (a RayleighDamping, or the two coefficients; the default (0, 0) is the undamped
        step bit for bit).  stiffness > 0 under Newmark or backward Euler covers the linear operators only (step raises FH_UNSUPPORTED
        otherwise); a_n is formed again after a change.  Returns self"""
        if isinstance(mass, RayleighDamping):
            mass, stiffness = mass.mass, mass.stiffness
        self._damping = (float(mass), float(stiffness))
        if self._h is not None:
            self._send_damping()
        return self

    def with_boundary_motion(self, direction, factor):
        """a prescribed motion of the Dirichlet nodes: at step n they hold u_n = u_0 + (factor[min(n, len - 1)] - factor[0]) direction, with
        u_0 the u of set_state (direction: one entry per dof, read on the Dirichlet dofs only; a numpy array or a device tensor; None
        clears the motion).  CentralDifference and BackwardEuler (without damping) cover it; step raises FH_UNSUPPORTED for Newmark.  v on
        the Dirichlet dofs is then the caller's: give set_state the slope of the table there, v_0 = (factor[1] - factor[0]) / dt direction.
        Returns self"""
        if direction is None:
            self._motion = (None, None)
        else:
            fac = _ffi.as_f64(factor).reshape(-1).copy()
            if len(fac) == 0:
                raise ValueError("factor needs at least one entry")
            self._motion = (direction if _is_torch(direction) else _ffi.as_f64(direction).reshape(-1).copy(), fac)
        if self._h is not None:
            self._send_motion()
        return self

    def _send_motion(self):
        if self._motion is None:
            return
        direction, fac = self._motion
        lib = self.engine._lib
        if direction is None:
            rc = lib.fh_dynamics_set_boundary_motion(self._h, None, None, 0)
        else:
            n = self._n()
            if (direction.numel() if _is_torch(direction) else np.size(direction)) != n:
                raise ValueError(f"direction must hold {n} entries")
            if _is_torch(direction):
                import torch

                dt_ = direction.to(dtype=torch.float64, device=f"cuda:{self.engine.device}").reshape(-1).contiguous()
                rc = lib.fh_dynamics_set_boundary_motion_dev(self._h, _ptr(dt_), _ffi.fp(fac), len(fac))
            else:
                rc = lib.fh_dynamics_set_boundary_motion(self._h, _ffi.fp(direction), _ffi.fp(fac), len(fac))
        self.engine._check(rc)

    def damping(self):
        """the RayleighDamping the handle uses"""
        h = self._handle()
        m, k = C.c_double(0.0), C.c_double(0.0)
        self.engine._check(self.engine._lib.fh_dynamics_damping(h, C.byref(m), C.byref(k)))
        return RayleighDamping(m.value, k.value)

    def _send_damping(self):
        if self._damping is not None:
            self.engine._check(self.engine._lib.fh_dynamics_set_damping(self._h, self._damping[0], self._damping[1]))

    def _bind(self, force=False):
        if force or getattr(self.engine, "_mf_bound", None) is not self:
            self.engine.set_operator_dirichlet_nodes(self._nodes)
            self.engine._mf_bound = self
        if force or getattr(self.engine, "_mass_bound", None) is not self:
            self.engine.set_mass_density(self._rho)
            self.engine._mass_bound = self
        _contact.bind_obstacles(self, force)

    def with_element_expansion(self, theta):
        """the per-element expansion of the engine (Engine.set_element_expansion: a scalar, one stretch per element, None to clear it).  The
        field belongs to the engine, not to this object: every object on the same engine sees it until it is changed.  The steps see a frozen field; changed
        between two step calls, the next call forms its starting acceleration (first order: rate) again; returns self"""
        self.engine.set_element_expansion(theta)
        return self

    def with_obstacles(self, obstacles):
        """the rigid obstacles of the penalty contact term (fenris_amd.contact.Obstacles; None: none): their force joins r(u) in every
        scheme and their energy the stored-energy column of the records; with friction on any of them the handle takes the Obstacles'
        slip_velocity (the first-order integrators refuse friction); returns self"""
        _contact.with_obstacles(self, obstacles)
        _contact.send_slip_velocity(self)
        return self

    def _n(self):
        return self.element_assembler.solution_dim() * self.engine.num_nodes()

    def _fh_settings(self):
        s = _ffi.DynamicsSettings()
        s.scheme, s.dt = self.scheme, self.dt
        s.newmark_beta, s.newmark_gamma = self._beta, self._gamma
        s.newton_tolerance, s.newton_max_iterations = self._settings.tolerance, self._settings.max_iterations or 0
        s.line_search = self._line_search.kind
        s.preconditioner = _ffi.PRECOND_MULTIGRID if self._mg is not None else _ffi.PRECOND_JACOBI
        s.linear_rel_tol, s.linear_max_iter = self._linear_rel_tol, self._linear_max_iter
        return s

    def _handle(self):
        self._bind()
        if self._h is None:
            h = C.c_void_p()
            s = self._fh_settings()
            self.engine._check(getattr(self.engine._lib, self._create)(self.engine._h, C.byref(s), C.byref(h)))
            self._h = h
            self._send_load()
            self._send_damping()
            self._send_motion()
            _contact.send_slip_velocity(self)
        return self._h

    def _drop(self):
        if self._h is not None:
            self.engine._lib.fh_dynamics_destroy(self._h)
            self._h = None

    def close(self):
        self._drop()

    def __del__(self):
        try:
            if getattr(self.engine, "_h", None):
                self._drop()
        except Exception:
            pass

    def _send_load(self):
        f, lf = self._load
        n = self._n()
        lib = self.engine._lib
        if f is not None and (f.numel() if _is_torch(f) else np.size(f)) != n:
            raise ValueError(f"f must hold {n} entries")
        cnt = 0 if lf is None else len(lf)
        if _is_torch(f):
            import torch

            ft = f.to(dtype=torch.float64, device=f"cuda:{self.engine.device}").reshape(-1).contiguous()
            rc = lib.fh_dynamics_set_load_dev(self._h, _ptr(ft), _ffi.fp(lf), cnt)
        else:
            fa = None if f is None else _ffi.as_f64(f).reshape(-1)
            rc = lib.fh_dynamics_set_load(self._h, _ffi.fp(fa), _ffi.fp(lf), cnt)
        self.engine._check(rc)

    # ---- state
    def set_state(self, u, v=None):
        """u_0 (with the Dirichlet values) and v_0 (None: zero): numpy arrays or device tensors; time and step count return to 0"""
        h = self._handle()
        n = self._n()
        lib = self.engine._lib
        for name, x in (("u", u), ("v", v)):
            if x is not None and (x.numel() if _is_torch(x) else np.size(x)) != n:
                raise ValueError(f"{name} must hold {n} entries")
        if _is_torch(u) or _is_torch(v):
            import torch

            dev = f"cuda:{self.engine.device}"
            ut = None if u is None else torch.as_tensor(u, dtype=torch.float64).to(dev).reshape(-1).contiguous()
            vt = None if v is None else torch.as_tensor(v, dtype=torch.float64).to(dev).reshape(-1).contiguous()
            rc = lib.fh_dynamics_set_state_dev(h, _ptr(ut), _ptr(vt))
        else:
            ua = None if u is None else _ffi.as_f64(u).reshape(-1)
            va = None if v is None else _ffi.as_f64(v).reshape(-1)
            rc = lib.fh_dynamics_set_state(h, _ffi.fp(ua), _ffi.fp(va))
        self.engine._check(rc)
        return self

    def step(self, num_steps, record_every=0):
        """num_steps steps; a record after every record_every steps and after the last (0: the last only).  Raises the Newton errors of
        MatrixFreeNewton for a failed implicit step, SingularJacobianError, and DynamicsError for everything else; each carries steps_done."""
        h = self._handle()
        if self._mg is not None:
            self._mg._bind(self._nodes, self._rho)
        num_steps, record_every = int(num_steps), int(record_every)
        rows = 1 + (num_steps // record_every if record_every else 0)
        rec = np.zeros((rows, 4))
        done = C.c_uint64(0)
        stats = np.zeros(5, dtype=np.uint64)
        rc = self.engine._lib.fh_dynamics_step(h, num_steps, record_every, _ffi.fp(rec), C.byref(done), _ffi.up(stats))
        k = int(stats[4])
        out = DynamicsRecord(rec[:k, 3].copy(), rec[:k, 0].copy(), rec[:k, 1].copy(), rec[:k, 2].copy(), int(done.value), tuple(int(x) for x in stats))
        if rc == _ffi.FH_OK:
            return out
        msg = self.engine.last_error()
        newton = {_ffi.FH_NEWTON_MAX_ITERATIONS: MaximumIterationsReached, _ffi.FH_NEWTON_JACOBIAN_ERROR: JacobianError,
                  _ffi.FH_NEWTON_LINE_SEARCH_FAILED: LineSearchError}
        if rc in newton:
            err = newton[rc](rc, msg, NewtonResult(int(stats[2]), int(stats[1]), int(stats[3]), 0, float("nan"), float("nan"), 0.0))
            err.steps_done, err.record = int(done.value), out
            raise err
        if rc == _ffi.FH_SINGULAR_JACOBIAN:
            err = SingularJacobianError(msg, -1)
            err.steps_done, err.record = int(done.value), out
            raise err
        err = DynamicsError(rc, msg, int(done.value))
        err.record = out
        raise err

    def state(self, device=False):
        """(u, v, a, time, step): numpy arrays, or device tensors with device=True"""
        h = self._handle()
        n = self._n()
        t, k = C.c_double(0.0), C.c_uint64(0)
        if device:
            import torch

            u, v, a = (torch.empty(n, dtype=torch.float64, device=f"cuda:{self.engine.device}") for _ in range(3))
            rc = self.engine._lib.fh_dynamics_state_dev(h, _ptr(u), _ptr(v), _ptr(a), C.byref(t), C.byref(k))
        else:
            u, v, a = np.zeros(n), np.zeros(n), np.zeros(n)
            rc = self.engine._lib.fh_dynamics_state(h, _ffi.fp(u), _ffi.fp(v), _ffi.fp(a), C.byref(t), C.byref(k))
        self.engine._check(rc)
        return u, v, a, t.value, int(k.value)

    def stable_dt(self, iterations=30):
        """(omega_max, dt_crit = 2 / omega_max; with stiffness damping (2 / omega_max)(sqrt(1 + xi^2) - xi), xi = stiffness omega_max / 2) from `iterations` steps of the power iteration on m^-1 T(u); the estimate of omega_max is a
        Rayleigh quotient and never too large, so dt_crit errs on the large side: apply a safety factor"""
        h = self._handle()
        om, dtc = C.c_double(0.0), C.c_double(0.0)
        self.engine._check(self.engine._lib.fh_dynamics_stable_dt(h, int(iterations), C.byref(om), C.byref(dtc)))
        return om.value, dtc.value


class CentralDifference(TimeIntegrator):
    """velocity-Verlet central differences with the row-sum lumped mass; the element kinds whose lumped mass has an entry that is not
    positive (Tet10, Tri6) are refused by step (FH_UNSUPPORTED)"""

    scheme = _ffi.DYN_CENTRAL_DIFFERENCE


class _Implicit(TimeIntegrator):
    def with_newton(self, settings=None, line_search=None, linear_rel_tol=1e-8, linear_max_iter=0):
        """the Newton solve of every step: NewtonSettings, NoLineSearch / BacktrackingLineSearch and the inner PCG's criterion; returns self"""
        self._settings = settings or NewtonSettings()
        self._line_search = line_search or BacktrackingLineSearch()
        self._linear_rel_tol, self._linear_max_iter = float(linear_rel_tol), int(linear_max_iter)
        self._drop()   # (the settings live in the handle: the state is set again afterwards)
        return self

    def with_multigrid(self, mg):
        """a GeometricMultigrid over this assembler: the steps' PCG then takes PRECOND_MULTIGRID; returns self"""
        self._mg = mg
        self._drop()
        return self


class Newmark(_Implicit):
    """Newmark(beta, gamma); the default (1/4, 1/2) is the average-acceleration (trapezoidal) rule"""

    scheme = _ffi.DYN_NEWMARK

    def __init__(self, element_assembler, density, dt, beta=0.25, gamma=0.5):
        super().__init__(element_assembler, density, dt)
        self._beta, self._gamma = float(beta), float(gamma)


class BackwardEuler(_Implicit):
    """backward Euler on positions: alpha = 1, beta = dt^2, u_ref = u_n + dt v_n"""

    scheme = _ffi.DYN_BACKWARD_EULER


@dataclass
class FirstOrderRecord(DynamicsRecord):
    """the records of a first-order step() call: column 0 (`kinetic`) holds 1/2 u^T B u, B the scheme's mass -- readable as mass_norm"""

    @property
    def mass_norm(self):
        return self.kinetic


class FirstOrderIntegrator(TimeIntegrator):
    """M du/dt + r(u) = lf_n f on the handle of fh_first_order_create.  The state is u alone: set_state takes no v, state() returns
    (u, rate, time, step) with rate = du/dt of the state as it stands, and step() returns a FirstOrderRecord."""

    _create = "fh_first_order_create"
    _stages, _theta = 1, 1.0

    def with_damping(self, mass=0.0, stiffness=0.0):
        raise TypeError("a first-order problem has no velocity to damp")

    def damping(self):
        raise TypeError("a first-order problem has no velocity to damp")

    def with_boundary_motion(self, direction, factor):
        raise TypeError("the first-order integrators do not cover a prescribed boundary motion")

    def _fh_settings(self):
        s = _ffi.FirstOrderSettings()
        s.scheme, s.dt, s.stages, s.theta = self.scheme, self.dt, self._stages, self._theta
        s.newton_tolerance, s.newton_max_iterations = self._settings.tolerance, self._settings.max_iterations or 0
        s.line_search = self._line_search.kind
        s.preconditioner = _ffi.PRECOND_MULTIGRID if self._mg is not None else _ffi.PRECOND_JACOBI
        s.linear_rel_tol, s.linear_max_iter = self._linear_rel_tol, self._linear_max_iter
        return s

    def step(self, num_steps, record_every=0):
        """as TimeIntegrator.step; the errors carry a FirstOrderRecord too"""
        def first_order(rec):
            return FirstOrderRecord(rec.time, rec.kinetic, rec.stored, rec.load_potential, rec.steps_done, rec.stats)

        try:
            return first_order(super().step(num_steps, record_every))
        except FenrisError as err:
            if hasattr(err, "record"):
                err.record = first_order(err.record)
            raise

    def state(self, device=False):
        """(u, rate, time, step): numpy arrays, or device tensors with device=True"""
        u, rate, _, time, step = super().state(device)
        return u, rate, time, step


class RungeKuttaLegendre(FirstOrderIntegrator):
    """Runge-Kutta-Legendre super-steps of `stages` stages with the row-sum lumped mass: stable for dt <= (stages^2 + stages) / lambda_max
    at the cost of `stages` residual passes (stable_dt returns that bound from a power iteration); the element kinds whose lumped mass has
    an entry that is not positive (Tet10, Tri6) are refused by step (FH_UNSUPPORTED)"""

    scheme = _ffi.FO_RKL

    def __init__(self, element_assembler, density, dt, stages=1):
        super().__init__(element_assembler, density, dt)
        self._stages = int(stages)

    def stable_dt(self, iterations=30):
        """(omega_max, dt_crit = (stages^2 + stages) / omega_max^2): omega_max^2 is a Rayleigh quotient of m^-1 T(u) and never too large, so
        dt_crit errs on the large side: apply a safety factor"""
        return super().stable_dt(iterations)


class ForwardEuler(RungeKuttaLegendre):
    """forward Euler: the one-stage Runge-Kutta-Legendre step, u_{n+1} = u_n + dt (lf_n f - r(u_n)) / m"""

    def __init__(self, element_assembler, density, dt):
        super().__init__(element_assembler, density, dt, stages=1)


class ThetaMethod(FirstOrderIntegrator, _Implicit):
    """the theta method with the consistent mass, 0.5 <= theta <= 1: Crank-Nicolson (the default 1/2) to implicit Euler (1); one Newton
    solve per step (with_newton, with_multigrid); stable_dt returns dt_crit = inf"""

    scheme = _ffi.FO_THETA

    def __init__(self, element_assembler, density, dt, theta=0.5):
        super().__init__(element_assembler, density, dt)
        self._theta = float(theta)
