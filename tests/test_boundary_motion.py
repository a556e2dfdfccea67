"""Prescribed motion of the Dirichlet nodes during time integration (fh_dynamics_set_boundary_motion, TimeIntegrator.with_boundary_motion)
against the NumPy statement of tests/motion_reference.py; meshes, problems and scenes are those of tests/test_moving_obstacles.py.

Tolerances: the bitwise statements are bitwise; every trajectory is held to motion_reference.measured_tolerance (d_perm from a permuted
connectivity, d_newton for backward Euler from a Newton tolerance 100 times smaller, 20 (d_perm + d_newton), floored at 1e-13), with the
CPU's figures in TRAJECTORY_TOLERANCE and a fresh measurement in every test that must stay within a factor 10 of them.  That the motion
adds no launch is read from fh_last_kernel_name (test_moving_obstacles.assert_step_route) beside the records' residual count.

Condition on the inputs, asserted on the reference: the moved nodes travel at least 1 % of the body's length.

Newmark with a boundary motion is out of scope (FH_UNSUPPORTED), so the statements "under every scheme" of this file cover central
differences and backward Euler; Newmark with moving obstacles alone is in tests/test_moving_obstacles.py."""
import ctypes as C

import numpy as np
import pytest

import fenris_amd as fa
from fenris_amd import _ffi

import motion_reference as mr
import test_moving_obstacles as tm
from test_moving_obstacles import EVERY, FH_BAD_ARGUMENT, FH_UNSUPPORTED, RHO, STEPS, engine  # noqa: F401  (engine: the fixture)

AMPLITUDE = 0.02     # of a body of length 1


def _motion(kind, shape="ramp"):
    """direction (1, 1/4, 1/8) on the clamped nodes; "ramp": g_n = AMPLITUDE (n / 16)^2, a smooth start; u_0 and v_0: the Dirichlet entries
    of u_0 are not zero (exactly representable), v_0 there is the slope of the table, the free nodes start at rest"""
    m = tm._mesh(kind)[0]
    N, d = m.vertices.shape
    dt = tm._modal(kind)["dt"]
    clamp = tm._clamp(m)
    direction = np.zeros((N, d))
    direction[clamp] = np.array([1.0, 0.25, 0.125])[:d]
    factor = AMPLITUDE * (np.arange(STEPS + 1) / STEPS) ** 2
    u0 = np.zeros((N, d))
    u0[clamp] = np.array([2.0 ** -8, -2.0 ** -9, 2.0 ** -10])[:d]
    v0 = ((factor[1] - factor[0]) / dt) * direction
    return direction.reshape(-1), factor, u0.reshape(-1), v0.reshape(-1)


def _eta_k(kind, damped):
    return 0.2 * tm._modal(kind)["dt"] if damped else 0.0


def _newton_tol(kind):
    """1e-10 of the inertia force scale m_min AMPLITUDE / dt^2 times dt^2"""
    return 1e-10 * tm._modal(kind)["m_min"] * AMPLITUDE


def _reference(oracle, kind, op, scheme, damped, perm=None, tol=0.0):
    direction, factor, u0, v0 = _motion(kind)
    prob = mr.Still(tm._problem(oracle, kind, op, perm=perm))
    dt = tm._modal(kind)["dt"]
    motion = mr.Motion(direction, factor)
    if scheme == "central":
        return mr.central_difference(prob, u0, v0, dt, STEPS, EVERY, motion=motion, eta_k=_eta_k(kind, damped))
    return mr.implicit(prob, scheme, u0, v0, dt, STEPS, EVERY, motion=motion, tol=tol)


def _measure(oracle, kind, op, scheme, damped):
    direction, factor, u0, _ = _motion(kind)
    travel = np.abs((factor[-1] - factor[0]) * direction).max()
    X = tm._mesh(kind)[0].vertices
    assert travel >= 0.01 * (X[:, 0].max() - X[:, 0].min())
    return mr.measured_tolerance(lambda perm, tol: _reference(oracle, kind, op, scheme, damped, perm, tol), _newton_tol(kind) if scheme != "central" else 0.0)


CASES = ([(k, "elastic", "central", k == "HEX8") for k in tm.KINDS] + [("HEX8", "neo_hookean", "central", True)]
         + [(k, "elastic", "euler", False) for k in ("HEX8", "TET4")])
# measured on the CPU with the reference alone (_measure): d_perm, d_newton and the tolerance 20 (d_perm + d_newton), floored at 1e-13
TRAJECTORY_TOLERANCE = {
    ('HEX8', 'elastic', 'central', True): (2.5e-14, 0.0e+00, 5.0e-13),
    ('TET4', 'elastic', 'central', False): (4.0e-14, 0.0e+00, 8.1e-13),
    ('QUAD4', 'elastic', 'central', False): (2.5e-14, 0.0e+00, 5.0e-13),
    ('TRI3', 'elastic', 'central', False): (4.0e-14, 0.0e+00, 8.0e-13),
    ('HEX8_776', 'elastic', 'central', False): (2.0e-14, 0.0e+00, 4.1e-13),
    ('HEX27', 'elastic', 'central', False): (6.3e-14, 0.0e+00, 1.3e-12),
    ('HEX8', 'neo_hookean', 'central', True): (3.7e-14, 0.0e+00, 7.4e-13),
    ('HEX8', 'elastic', 'euler', False): (2.5e-13, 0.0e+00, 5.0e-12),
    ('TET4', 'elastic', 'euler', False): (9.2e-14, 0.0e+00, 1.8e-12),
}


def _moved_integrator(engine, kind, op, scheme, damped, motion=True, obstacles=None, state=None):
    """the integrator on a new assembler, its state set"""
    direction, factor, u0, v0 = _motion(kind) if state is None else state
    dt = tm._modal(kind)["dt"]
    ti = tm._integrator(scheme, tm._assembler(engine, kind, op), kind, dt, newton_tol=_newton_tol(kind))
    if obstacles is not None:
        ti.with_obstacles(obstacles)
    if damped:
        ti.with_damping(0.0, _eta_k(kind, True))
    if motion:
        ti.with_boundary_motion(direction, factor)
    ti.set_state(u0, v0)
    return ti


def _device(engine, kind, op, scheme, damped, cuts=(STEPS,), motion=True, obstacles=None, state=None):
    ti = _moved_integrator(engine, kind, op, scheme, damped, motion, obstacles, state)
    rows = []
    for count in cuts:
        rec = ti.step(count, record_every=EVERY if len(cuts) == 1 else 0)
        assert rec.steps_done == count
        rows.append(tm._records(rec))
    u, v, a, _, step = ti.state()
    assert step == sum(cuts)
    return (u, v, a, np.concatenate(rows)), ti


# ------------------------------------------------------------------------------------------ GPU 5: trajectories
@pytest.mark.gpu
@pytest.mark.parametrize("kind,op,scheme,damped", CASES)
def test_trajectory_with_boundary_motion(engine, oracle, kind, op, scheme, damped):
    """16 steps with a record every 4 while the clamped face is pulled along a quadratic ramp: u, v, a and the records against the
    reference; the Dirichlet entries of u are fma(g_n - g_0, direction, u_0) to the bit.  With stiffness damping the boundary's half-step
    velocity enters the damping force of its neighbours"""
    ref, d_perm, d_newton, tol = _measure(oracle, kind, op, scheme, damped)
    tol = mr.check_constants(TRAJECTORY_TOLERANCE, (kind, op, scheme, damped), d_perm, d_newton, tol)
    if damped:      # ... and it matters: the undamped reference differs
        plain = _reference(oracle, kind, op, scheme, False)
        assert mr.rel_diff(ref, plain) > 1e-3
    got, ti = _device(engine, kind, op, scheme, damped)
    mr.assert_parity(got, ref, tol, f"{kind} {op} {scheme} damped={damped}")
    direction, factor, u0, _ = _motion(kind)
    fixed = direction != 0.0
    assert fixed.any() and np.array_equal(got[0][fixed], mr.Motion(direction, factor).u(STEPS, u0)[fixed])
    assert np.abs(got[0][fixed] - u0[fixed]).max() >= 0.01
    if scheme == "central":     # a stored state: the boundary keeps its half-step velocity and has a = 0
        assert np.array_equal(got[1][fixed], mr.Motion(direction, factor).half_velocity(STEPS - 1, tm._modal(kind)["dt"])[fixed])
        assert not got[2][fixed].any()
        ti.close()      # no launch is added for the motion: the step's launch is the one it was
        t2 = _moved_integrator(engine, kind, op, scheme, damped)
        tm.assert_step_route(engine, t2, kind, contact=False, damped=damped)
        t2.close()


# ------------------------------------------------------------------------------------------ GPU 6: rigid translation
RIGID_TOLERANCE = {
    'central': (4.5e-17, 0.0e+00, 1.0e-13),
    'euler': (1.4e-17, 0.0e+00, 1.0e-13),
}


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["central", "euler"])
def test_rigid_translation(engine, oracle, scheme):
    """the clamped nodes move at a constant velocity V and the free nodes start with v_0 = V: the body translates.  u - n dt V stays
    within the measured tolerance of |n dt V|; the stored energy stays at rounding level: displacement errors of tol |u| over an element of
    size h are strains of tol |u| / h, an energy density of at most 4 mu of their square (lambda < 2 mu here)"""
    kind = "HEX8"
    m = tm._mesh(kind)[0]
    N, d = m.vertices.shape
    dt = tm._modal(kind)["dt"]
    V = np.array([0.5, -0.25, 0.125])
    direction = np.tile(V, N)
    factor = np.arange(STEPS + 1) * dt
    state = (direction, factor, np.zeros(N * d), direction.copy())
    motion = mr.Motion(direction, factor)

    def run(perm, tol):
        prob = mr.Still(tm._problem(oracle, kind, "elastic", perm=perm))
        if scheme == "central":
            return mr.central_difference(prob, state[2], state[3], dt, STEPS, EVERY, motion=motion)
        return mr.implicit(prob, scheme, state[2], state[3], dt, STEPS, EVERY, motion=motion, tol=tol)

    ref, d_perm, d_newton, tol = mr.measured_tolerance(run, _newton_tol(kind) if scheme != "central" else 0.0)
    tol = mr.check_constants(RIGID_TOLERANCE, scheme, d_perm, d_newton, tol)
    got, ti = _device(engine, kind, "elastic", scheme, False, state=state)
    exact = STEPS * dt * direction
    for name, x in (("reference", ref), ("device", got)):
        err = np.abs(x[0] - exact).max() / np.abs(exact).max()
        print(f"rigid translation {scheme} {name}: |u - n dt V| {err:.3e} (tol {tol:.3e}), stored energy {np.abs(x[3][:, 1]).max():.3e}")
    assert np.abs(got[0] - exact).max() <= tol * np.abs(exact).max()
    for name, p, q in zip("uv", got[:2], ref[:2]):      # (a is rounding noise around zero in both)
        tm._check(f"rigid {scheme} {name}", tm._rel(p, q), tol)
    h = 1.0 / 3.0
    assert np.abs(got[3][:, 1]).max() <= 4.0 * tm.LAME.mu * 1.0 * (tol * np.abs(exact).max() / h) ** 2


# ------------------------------------------------------------------------------------------ GPU 7: cuts, both motions and friction
@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["central", "euler"])
def test_cut_runs_with_both_motions_repeat_bit_for_bit(scheme):
    """a sliding frictional floor and a pulled clamp: 16 steps in one call against 5 + 1 + 10, and a second identical run: identical bits"""
    kind = "HEX8"
    obs, paths, mu, eps_v = tm._scene(kind, "belt")

    def run(cuts):
        eng = fa.Engine(0)
        try:
            got, ti = _device(eng, kind, "neo_hookean", scheme, False, cuts, obstacles=tm._fa_obstacles(obs, mu, paths, slip_velocity=eps_v))
            if scheme == "central":      # both motions and friction: still the element pass and the fused node pass
                ti.close()
                t2 = _moved_integrator(eng, kind, "neo_hookean", scheme, False, obstacles=tm._fa_obstacles(obs, mu, paths, slip_velocity=eps_v))
                tm.assert_step_route(eng, t2, kind, contact=True)
                t2.close()
            return got[0], got[1], got[2], got[3][-1]
        finally:
            eng.close()

    base = run((STEPS,))
    assert np.isfinite(base[0]).all() and np.abs(base[0]).max() >= 0.01
    for cuts in ((STEPS,), (5, 1, 10)):
        for name, p, q in zip("uvar", base, run(cuts)):
            assert np.array_equal(p, q), (scheme, cuts, name)


# ------------------------------------------------------------------------------------------ GPU 8: off means off (the boundary motion)
@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["central", "euler"])
def test_a_motion_that_does_not_move_changes_no_bit(scheme):
    """a boundary motion with zero direction, and one with a constant factor table, over a frictional floor: the bits of a run that never
    made the call (v_0 is zero on the Dirichlet dofs, which a motion no longer zeroes itself)"""
    kind = "HEX8"
    obs, _, mu, eps_v = tm._scene(kind, "belt")
    direction, factor, _, _ = _motion(kind)
    n = len(direction)
    v0 = np.where(direction != 0.0, 0.0, 0.05 * np.random.default_rng(3).uniform(-1.0, 1.0, n))

    def run(which):
        eng = fa.Engine(0)
        try:
            state = {"none": None, "zero direction": (np.zeros(n), factor, np.zeros(n), v0),
                     "constant table": (direction, np.full(5, 0.375), np.zeros(n), v0)}[which]
            got, _ = _device(eng, kind, "neo_hookean", scheme, False, motion=which != "none", obstacles=tm._fa_obstacles(obs, mu, None, slip_velocity=eps_v),
                             state=state if state is not None else (direction, factor, np.zeros(n), v0))
            con = fa.Contact(eng)
            return list(got) + [con.force(), con.friction_force()]
        finally:
            eng.close()

    plain = run("none")
    assert np.abs(plain[4]).max() > 0.0 and np.abs(plain[5]).max() > 0.0
    for which in ("zero direction", "constant table"):
        for i, (p, q) in enumerate(zip(plain, run(which))):
            assert np.array_equal(p, q), (which, i)


# ------------------------------------------------------------------------------------------ GPU 10: arguments and scope
@pytest.mark.gpu
def test_arguments_and_scope(engine):
    kind = "HEX8"
    direction, factor, u0, v0 = _motion(kind)
    dt = tm._modal(kind)["dt"]
    asm = tm._assembler(engine, kind, "elastic")
    lib = engine._lib
    ti = tm._integrator("central", asm, kind, dt)
    h = ti._handle()
    for bad in ((_ffi.fp(direction), _ffi.fp(factor), 0), (_ffi.fp(direction), None, 3), (_ffi.fp(direction), _ffi.fp(np.array([0.0, np.nan])), 2)):
        assert lib.fh_dynamics_set_boundary_motion(h, *bad) == FH_BAD_ARGUMENT
    ti.set_state(u0, v0)
    plain = ti.step(2)                                   # ... and no motion was set by the refused calls
    assert np.array_equal(ti.state()[0][direction != 0.0], u0[direction != 0.0])
    ti.with_boundary_motion(direction, factor).set_state(u0, v0)
    ti.step(2)
    assert not np.array_equal(ti.state()[0][direction != 0.0], u0[direction != 0.0])
    ti.with_boundary_motion(None, None).set_state(u0, v0)      # NULL clears it
    again = ti.step(2)
    assert np.array_equal(ti.state()[0][direction != 0.0], u0[direction != 0.0]) and np.array_equal(tm._records(plain), tm._records(again))
    ti.close()
    # out of scope: Newmark; backward Euler with damping; a first-order handle -- from step and from state, the state left as it was
    refused = [tm._integrator("newmark", asm, kind, dt).with_boundary_motion(direction, factor),
               tm._integrator("euler", asm, kind, dt).with_damping(0.1, 0.0).with_boundary_motion(direction, factor)]
    for ti in refused:
        ti.set_state(u0, v0)
        assert tm._code(ti.step, 2) == FH_UNSUPPORTED and "boundary motion" in engine.last_error()
        assert tm._code(ti.state) == FH_UNSUPPORTED
        ti.with_boundary_motion(None, None)
        u, _, _, _, step = ti.state()
        assert step == 0 and np.array_equal(u, u0)
        ti.close()
    with pytest.raises(TypeError):
        fa.ForwardEuler(asm, RHO, 1e-4).with_boundary_motion(direction, factor)
    fo = fa.ForwardEuler(asm, RHO, 1e-4)
    fo.set_state(u0)
    assert lib.fh_dynamics_set_boundary_motion(fo._handle(), _ffi.fp(direction), _ffi.fp(factor), len(factor)) == 0
    done, stats = C.c_uint64(0), np.zeros(5, dtype=np.uint64)
    assert lib.fh_dynamics_step(fo._handle(), 1, 0, _ffi.fp(np.zeros(4)), C.byref(done), _ffi.up(stats)) == FH_UNSUPPORTED and done.value == 0
    assert lib.fh_dynamics_set_boundary_motion(fo._handle(), None, None, 0) == 0
    assert tm._code(fo.step, 1) == 0
    fo.close()
