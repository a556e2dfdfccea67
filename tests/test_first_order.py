"""First-order time integration on the device (fh_first_order_create, fenris_amd.dynamics): Runge-Kutta-Legendre super-steps (one stage:
forward Euler) and the theta method against the NumPy statement of tests/first_order_reference.py, which is pinned here on the CPU against
the closed forms of a single eigenmode.  Meshes, clamp, loads and assemblers are those of tests/test_dynamics.py."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import fenris_amd as fa
from fenris_amd import _ffi

import first_order_reference as fr
import test_dynamics as td

RHO = td.RHO
FH_BAD_ARGUMENT, FH_INVALID_STATE, FH_UNSUPPORTED, FH_DYNAMICS_NONFINITE = 2, 5, 6, 15
RKL_STAGES, THETAS, COUNTS = (1, 2, 5), (0.5, 1.0), (1, 2, 7, 32)
LINEAR_CASES = [("rkl", 1), ("rkl", 2), ("rkl", 5), ("theta", 0.5), ("theta", 1.0)]
LINEAR_REL_TOL = 1e-12


@pytest.fixture()
def engine():
    eng = fa.Engine(0)
    yield eng
    eng.close()


def _id(case):
    return f"{case[0]}{case[1]:g}"


# ------------------------------------------------------------------------------------------ problems, integrators
@functools.lru_cache(maxsize=None)
def _modal(kind, op):
    """dense pencils of the clamped body at u = 0: all modes of (K, diag m) (of (K, M) where the lumped mass is not positive), the lowest
    mode of (K, M), dt_theta = 0.05 / lambda_0 of (K, M) and the condition numbers of M + theta dt_theta K on the free dofs"""
    from oracle import oracle as o

    o.lib()
    prob = td._problem(o, kind, op)
    z = np.zeros(prob.n)
    wc, Vc = fr.dense_pencil(prob, z, False)
    lumped_ok = (prob.lumped()[prob.free] > 0).all()
    wl, Vl = fr.dense_pencil(prob, z, True) if lumped_ok else (wc, Vc)
    free = prob.free
    K0 = prob.tangent(z)
    K, M = K0[free][:, free].toarray(), prob.mass()[free][:, free].toarray()
    dt_theta = 0.05 / wc[0]
    return {"wl": wl, "Vl": Vl, "lam_max": wl[-1], "lam0": wc[0], "phi0": Vc[:, 0], "dt_theta": dt_theta, "K0": K0,
            "kappa": {th: np.linalg.cond(M + th * dt_theta * K) for th in THETAS}}


def _dt(md, case, safety):
    """RKL: safety (s^2 + s) / lambda_max of (K, diag m); theta: 0.05 / lambda_0 of (K, M)"""
    if case[0] == "rkl":
        s = case[1]
        return safety * (s * s + s) / md["lam_max"]
    return md["dt_theta"]


def _bound(md, case, steps):
    """RKL: rounding only (the map contracts), 1e-10; theta: 10 steps kappa(M + theta dt K) linear_rel_tol"""
    return 1e-10 if case[0] == "rkl" else 10.0 * steps * md["kappa"][case[1]] * LINEAR_REL_TOL


def _integrator(case, asm, kind, dt, f=None, load_factor=None, newton_tol=1e-8, max_it=None, rho=RHO, linear_rel_tol=LINEAR_REL_TOL):
    clamp = td._clamp(td._mesh(kind)[0])
    if case[0] == "rkl":
        ti = fa.ForwardEuler(asm, rho, dt) if case[1] == 1 else fa.RungeKuttaLegendre(asm, rho, dt, stages=case[1])
    else:
        ti = fa.ThetaMethod(asm, rho, dt, theta=case[1]).with_newton(fa.NewtonSettings(max_it, newton_tol), linear_rel_tol=linear_rel_tol)
    return ti.with_dirichlet_nodes(clamp).with_load(f, load_factor)


def _reference_run(prob, case, u0, dt, steps, record_every, tol=1e-8):
    if case[0] == "rkl":
        return fr.rkl(prob, u0, dt, case[1], steps, record_every)
    st, u, rate, rec, done, _ = fr.theta_method(prob, u0, dt, case[1], steps, record_every, tol=tol)
    assert st == "ok" and done == steps
    return u, rate, rec


def _rel_diff(x, y):
    """the largest difference over (u, rate, every record column), each relative to the first trajectory's largest magnitude"""
    out = 0.0
    for p, q in zip(x[:2], y[:2]):
        out = max(out, np.abs(p - q).max() / max(np.abs(p).max(), 1e-300))
    for c in range(4):
        out = max(out, np.abs(x[2][:, c] - y[2][:, c]).max() / max(np.abs(x[2][:, c]).max(), 1e-300))
    return out


def _assert_parity(got, ref, tol, what=""):
    for name, p, q in zip(("u", "rate"), got[:2], ref[:2]):
        err = np.abs(p - q).max() / max(np.abs(q).max(), 1e-300)
        print(f"{what} {name}: {err:.3e} (tol {tol:.3e})")
        assert err <= tol, (what, name, err, tol)
    for c, name in enumerate(("mass_norm", "stored", "load_potential", "time")):
        err = np.abs(got[2][:, c] - ref[2][:, c]).max() / max(np.abs(ref[2][:, c]).max(), 1e-300)
        print(f"{what} {name}: {err:.3e} (tol {tol:.3e})")
        assert err <= tol, (what, name, err, tol)


def _records(rec):
    return np.stack([rec.mass_norm, rec.stored, rec.load_potential, rec.time], axis=1)


# ------------------------------------------------------------------------------------------ 1, 2. no GPU: declarations, the reference pinned
def test_first_order_entry_point_is_declared():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fenris_hip.h")).read()
    assert "fh_first_order_create" in _ffi.exported_symbols() and "fh_first_order_create(" in hdr
    for text in ("FH_FO_RKL = 0, FH_FO_THETA = 1", "} fh_first_order_settings;", "#define FH_ABI_VERSION 1",
                 "FH_DYN_CENTRAL_DIFFERENCE = 0, FH_DYN_BACKWARD_EULER = 1, FH_DYN_NEWMARK = 2", "} fh_dynamics_settings;"):
        assert text in hdr
    for cls in (fa.FirstOrderIntegrator, fa.RungeKuttaLegendre, fa.ForwardEuler, fa.ThetaMethod):
        assert issubclass(cls, fa.TimeIntegrator)
    assert issubclass(fa.ForwardEuler, fa.RungeKuttaLegendre) and issubclass(fa.FirstOrderRecord, fa.DynamicsRecord)
    assert (_ffi.FO_RKL, _ffi.FO_THETA) == (0, 1)
    rec = fa.FirstOrderRecord(np.zeros(1), np.ones(1), np.zeros(1), np.zeros(1), 1, (1, 1, 0, 0, 1))
    assert rec.mass_norm is rec.kinetic


def test_closed_forms_on_a_random_pencil():
    """both identities on a random 12-dof pencil, the recurrences written out with dense matrices"""
    rng = np.random.default_rng(11)
    A = rng.standard_normal((12, 12))
    K = A @ A.T + 12.0 * np.eye(12)
    m = rng.uniform(0.5, 2.0, 12)
    B = rng.standard_normal((12, 12))
    M = B @ B.T + 12.0 * np.eye(12)
    import scipy.linalg as sl

    wl, Vl = sl.eigh(K, np.diag(m))
    wc, Vc = sl.eigh(K, M)
    for s in RKL_STAGES:
        dt, w1 = 0.45 * (s * s + s) / wl[-1], 2.0 / (s * s + s)
        for mode in (0, 6):
            u = Vl[:, mode].copy()
            for n in range(1, 33):
                prev, cur = u, u - w1 * dt * (K @ u) / m
                for k in range(2, s + 1):
                    mu, nu = (2.0 * k - 1.0) / k, (1.0 - k) / k
                    prev, cur = cur, mu * cur + nu * prev - mu * w1 * dt * (K @ cur) / m
                u = cur
                assert np.abs(u - fr.closed_form("rkl", wl[mode], dt, n, stages=s) * Vl[:, mode]).max() <= 1e-14 * np.abs(Vl[:, mode]).max()
    for theta in THETAS:
        dt = 0.05 / wc[0]
        u = Vc[:, 0].copy()
        for n in range(1, 33):
            u = np.linalg.solve(M + theta * dt * K, M @ u - (1.0 - theta) * dt * (K @ u))
            assert np.abs(u - fr.closed_form("theta", wc[0], dt, n, theta=theta) * Vc[:, 0]).max() <= 1e-14 * np.abs(Vc[:, 0]).max()


@pytest.mark.parametrize("case", LINEAR_CASES, ids=_id)
@pytest.mark.parametrize("kind,op", [("HEX8_SMALL", "elastic"), ("TET4_SMALL", "elastic"), ("QUAD4_SMALL", "laplace")])
def test_reference_meets_the_closed_forms(oracle, kind, op, case):
    """u_0 = phi, f = 0 on one eigenmode of the scheme's dense pencil: u_n = c_n phi to 1e-10 max|phi| for n in (1, 2, 7, 32) -- RKL at
    dt = 0.45 (s^2 + s) / lambda_max on the lowest and the median mode of (K, diag m), theta at dt = 0.05 / lambda_0 on the lowest mode of (K, M)"""
    md = _modal(kind, op)
    prob = td._problem(oracle, kind, op)
    dt = _dt(md, case, 0.45)
    if case[0] == "rkl":
        modes = [(md["wl"][k], md["Vl"][:, k]) for k in (0, len(md["wl"]) // 2)]
    else:
        modes = [(md["lam0"], md["phi0"])]
    for lam, phi in modes:
        tol_n = 1e-12 * case[1] * dt * np.linalg.norm(md["K0"] @ phi)
        for n in COUNTS:
            u = _reference_run(prob, case, phi, dt, n, 0, tol=tol_n)[0]
            want = fr.closed_form(case[0], lam, dt, n, stages=case[1], theta=case[1]) * phi
            assert np.abs(u - want).max() <= 1e-10 * np.abs(phi).max()


# ------------------------------------------------------------------------------------------ 3. single-mode closed forms on the device
@pytest.mark.gpu
@pytest.mark.parametrize("case", LINEAR_CASES, ids=_id)
@pytest.mark.parametrize("kind,op", [("HEX8", "elastic"), ("TET4", "elastic"), ("QUAD4", "laplace")])
def test_single_mode_closed_forms(engine, kind, op, case):
    """the cases of the reference's test, 32 steps taken one at a time and compared after every one.  RKL involves rounding only (the map
    contracts): 1e-10 max|phi|; theta solves to linear_rel_tol = 1e-12: 10 steps kappa(M + theta dt K) linear_rel_tol"""
    md = _modal(kind, op)
    dt, steps = _dt(md, case, 0.45), 32
    tol = _bound(md, case, steps)
    if case[0] == "rkl":
        modes = [(md["wl"][k], md["Vl"][:, k]) for k in (0, len(md["wl"]) // 2)]
    else:
        modes = [(md["lam0"], md["phi0"])]
    asm = td._assembler(engine, kind, op)
    for lam, phi in modes:
        ti = _integrator(case, asm, kind, dt, newton_tol=1e-11 * case[1] * dt * np.linalg.norm(md["K0"] @ phi))
        ti.set_state(phi)
        worst = 0.0
        for n in range(1, steps + 1):
            rec = ti.step(1)
            assert rec.steps_done == 1 and len(rec.time) == 1 and abs(rec.time[0] - n * dt) <= 1e-14 * n * dt
            u = ti.state()[0]
            want = fr.closed_form(case[0], lam, dt, n, stages=case[1], theta=case[1]) * phi
            worst = max(worst, np.abs(u - want).max() / np.abs(phi).max())
        print(f"{kind} {op} {_id(case)} lambda dt {lam * dt:.3e}: worst error {worst:.3e} of max|phi| (tol {tol:.3e})")
        assert worst <= tol
        ti.close()


# ------------------------------------------------------------------------------------------ 4. invariants, linear operators
@functools.lru_cache(maxsize=None)
def _static(kind, op):
    """a constant body load sized so that the static solution K u* = f is as large as the lowest mode, and u*"""
    from oracle import oracle as o

    md = _modal(kind, op)
    m = td._mesh(kind)[0]
    if op == "laplace":
        f = np.full(m.num_nodes(), 1.0 / m.num_nodes())
        f[td._clamp(m)] = 0.0
    else:
        f = td._body_load(kind, 1.0)
    prob = td._problem(o, kind, op, direct="sparse")
    us = prob.solve_free(md["K0"], f)
    scale = np.abs(md["phi0"]).max() / np.abs(us).max()
    return scale * f, scale * us


@pytest.mark.gpu
@pytest.mark.parametrize("case", [("rkl", 1), ("rkl", 5), ("theta", 0.5), ("theta", 1.0)], ids=_id)
@pytest.mark.parametrize("kind,op", [("HEX8", "elastic"), ("TET4", "elastic"), ("QUAD4", "laplace"), ("TRI3", "laplace")])
def test_invariants_of_the_linear_schemes(engine, oracle, kind, op, case):
    """a constant body load, 64 steps recorded every step, RKL at dt = 0.9 (s^2 + s) / lambda_max.  From the lowest mode the potential
    stored - load_potential never rises by more than the bound of the single-mode test relative to its first value, and ends lower; from
    the static solution K u* = f the state stays at u* within the same bound"""
    md = _modal(kind, op)
    dt, steps = _dt(md, case, 0.9), 64
    bound = _bound(md, case, steps)
    f, us = _static(kind, op)
    u0 = md["phi0"]
    tol_n = 1e-11 * case[1] * dt * np.linalg.norm(f)
    ti = _integrator(case, td._assembler(engine, kind, op), kind, dt, f, newton_tol=tol_n)
    ti.set_state(u0)
    rec = ti.step(steps, record_every=1)
    assert len(rec.time) == steps
    prob = td._problem(oracle, kind, op)
    P = np.concatenate([[prob.energy(u0) - float(f @ u0)], rec.stored - rec.load_potential])
    rise = np.max(np.diff(P)) / abs(P[0])
    print(f"{kind} {op} {_id(case)}: largest relative rise of the potential {rise:.3e} (bound {bound:.3e}), P_0 {P[0]:.4e}, P_64 {P[-1]:.4e}")
    assert rise <= bound and P[-1] < P[0]
    ti.set_state(us)
    ti.step(steps)
    u = ti.state()[0]
    drift = np.abs(u - us).max() / np.abs(us).max()
    print(f"{kind} {op} {_id(case)}: drift from the static solution {drift:.3e} (bound {bound:.3e})")
    assert drift <= bound


# ------------------------------------------------------------------------------------------ 5. trajectory parity, nonlinear
NONLINEAR_CASES = [("rkl", 1), ("rkl", 4), ("theta", 0.5), ("theta", 1.0)]
SHEAR = 0.15
# Measured on the CPU with the reference alone (_measured_tolerance): d_perm, d_newton and the resulting tolerance 20 (d_perm + d_newton),
# floored at 1e-13, per (mesh, material, scheme).  The test measures them again and asserts that they stay within a factor 10 of these.
TRAJECTORY_TOLERANCE = {
    ("HEX8", "neo_hookean", "rkl1"): (8.6e-15, 0.0e+00, 1.7e-13),
    ("HEX8", "neo_hookean", "rkl4"): (6.6e-14, 0.0e+00, 1.3e-12),
    ("HEX8", "neo_hookean", "theta0.5"): (1.7e-13, 7.7e-11, 1.5e-09),
    ("HEX8", "neo_hookean", "theta1"): (1.2e-12, 1.4e-12, 5.2e-11),
    ("HEX8", "stvk", "rkl1"): (8.0e-15, 0.0e+00, 1.6e-13),
    ("HEX8", "stvk", "rkl4"): (9.3e-14, 0.0e+00, 1.9e-12),
    ("HEX8", "stvk", "theta0.5"): (1.2e-13, 9.6e-12, 1.9e-10),
    ("HEX8", "stvk", "theta1"): (1.7e-12, 1.4e-12, 6.2e-11),
    ("TET4", "neo_hookean", "rkl1"): (7.6e-15, 0.0e+00, 1.5e-13),
    ("TET4", "neo_hookean", "rkl4"): (7.4e-14, 0.0e+00, 1.5e-12),
    ("TET4", "neo_hookean", "theta0.5"): (7.8e-14, 3.2e-11, 6.3e-10),
    ("TET4", "neo_hookean", "theta1"): (1.4e-13, 0.0e+00, 2.8e-12),
    ("TET4", "stvk", "rkl1"): (5.9e-15, 0.0e+00, 1.2e-13),
    ("TET4", "stvk", "rkl4"): (6.7e-14, 0.0e+00, 1.3e-12),
    ("TET4", "stvk", "theta0.5"): (8.3e-14, 1.7e-11, 3.3e-10),
    ("TET4", "stvk", "theta1"): (1.6e-13, 1.5e-13, 6.1e-12),
}


def _shear(kind, amount=SHEAR):
    """a smooth finite initial deformation: the free end sheared along y by `amount` of the body's length, nothing on the clamped face
    (u_y depends on x alone: det F = 1 everywhere)"""
    m = td._mesh(kind)[0]
    x = m.vertices[:, 0]
    L = x.max() - x.min()
    d = m.vertices.shape[1]
    u = np.zeros(d * m.num_nodes())
    u[1::d] = amount * L * np.sin(0.5 * np.pi * (x - x.min()) / L)
    return u


def _nonlinear_dt(kind, case):
    """RKL: half the stability bound of the unloaded body (the sheared one is stiffer); theta: 0.05 of the slowest relaxation time"""
    return _dt(_modal(kind, "elastic"), case, 0.5)


def _newton_tol(prob, case, u0, dt):
    """1e-11 theta dt |r(u_0)| on the free dofs: the reference and the device both stop some orders above the rounding of F"""
    if case[0] == "rkl":
        return 0.0
    return 1e-11 * case[1] * dt * np.linalg.norm(prob.residual(u0)[prob.free])


def _measured_tolerance(oracle, kind, op, case, f, lf, u0, dt, steps, every, tol, kw=None, kw_perm=None):
    """the reference against itself, as in tests/test_dynamics.py: d_perm from a permuted connectivity (another summation order in r),
    d_newton from a Newton tolerance 100 times smaller; tolerance 20 (d_perm + d_newton), never below 1e-13"""
    kw = dict(kw or {"direct": "sparse"})
    kwp = dict(kw if kw_perm is None else kw_perm)
    ref = _reference_run(td._problem(oracle, kind, op, f, lf, **kw), case, u0, dt, steps, every, tol)
    base = ref if kw_perm is None else _reference_run(td._problem(oracle, kind, op, f, lf, **kwp), case, u0, dt, steps, every, tol)
    perm = _reference_run(td._problem(oracle, kind, op, f, lf, perm=7, **kwp), case, u0, dt, steps, every, tol)
    d_perm = _rel_diff(base, perm)
    d_newton = 0.0
    if case[0] == "theta":
        d_newton = _rel_diff(ref, _reference_run(td._problem(oracle, kind, op, f, lf, **kw), case, u0, dt, steps, every, tol / 100.0))
    return ref, d_perm, d_newton, max(20.0 * (d_perm + d_newton), 1e-13)


@pytest.mark.parametrize("case", NONLINEAR_CASES, ids=_id)
@pytest.mark.parametrize("op", ["neo_hookean", "stvk"])
@pytest.mark.parametrize("kind", ["HEX8", "TET4"])
def test_nonlinear_trajectories_sit_in_the_nonlinear_range(oracle, kind, op, case):
    """the condition of the parity test, on the reference alone: the trajectory differs from the LinearElastic one by more than 100 times
    the parity tolerance, and no point inverts (every stored energy and the final rate are finite)"""
    dt = _nonlinear_dt(kind, case)
    f, lf, u0 = td._body_load(kind, td.LOAD[kind]), td._ramp(), _shear(kind)
    prob = td._problem(oracle, kind, op, f, lf, direct="sparse")
    lin = td._problem(oracle, kind, "elastic", f, lf, direct="sparse")
    tol_n = _newton_tol(prob, case, u0, dt)
    ref = _reference_run(prob, case, u0, dt, 16, 4, tol_n)
    linear = _reference_run(lin, case, u0, dt, 16, 4, tol_n)
    assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all() and np.isfinite(ref[2]).all()
    gap = _rel_diff(ref, linear)
    print(f"{kind} {op} {_id(case)}: nonlinear against linear {gap:.3e}, tolerance {TRAJECTORY_TOLERANCE[(kind, op, _id(case))][2]:.3e}")
    assert gap > 100.0 * TRAJECTORY_TOLERANCE[(kind, op, _id(case))][2]


@pytest.mark.gpu
@pytest.mark.parametrize("case", NONLINEAR_CASES, ids=_id)
@pytest.mark.parametrize("op", ["neo_hookean", "stvk"])
@pytest.mark.parametrize("kind", ["HEX8", "TET4"])
def test_trajectory_parity_with_the_reference(engine, oracle, kind, op, case):
    """16 steps from the sheared state under the ramped load with a record every 4: u, the rate and every record row against the reference"""
    dt = _nonlinear_dt(kind, case)
    f, lf, u0 = td._body_load(kind, td.LOAD[kind]), td._ramp(), _shear(kind)
    tol_n = _newton_tol(td._problem(oracle, kind, op, f, lf), case, u0, dt)
    ref, d_perm, d_newton, tol = _measured_tolerance(oracle, kind, op, case, f, lf, u0, dt, 16, 4, tol_n)
    tol = td._check_constants((kind, op, _id(case)), d_perm, d_newton, tol, TRAJECTORY_TOLERANCE)
    ti = _integrator(case, td._assembler(engine, kind, op), kind, dt, f, lf, newton_tol=tol_n)
    ti.set_state(u0)
    rec = ti.step(16, record_every=4)
    assert rec.steps_done == 16 and len(rec.time) == 4 and rec.stats[0] == 16 and rec.stats[4] == 4
    u, rate, time, step = ti.state()
    assert step == 16 and abs(time - 16 * dt) <= 1e-14 * time
    _assert_parity((u, rate, _records(rec)), ref, tol, f"{kind} {op} {_id(case)}")
    if case[0] == "rkl":
        assert engine.last_kernel_name() == "k_element_pass_tiled + k_first_order_from_partials"


# ------------------------------------------------------------------------------------------ 6. the other routes
# measured like TRAJECTORY_TOLERANCE, per case
OTHER_TOLERANCE = {
    "hex27_rkl3": (1.2e-13, 0.0e+00, 2.5e-12),
    "tet10_theta0.5": (5.0e-14, 3.1e-11, 6.3e-10),
    "rules_rkl2": (1.4e-14, 0.0e+00, 2.9e-13),
    "rules_theta1": (7.6e-14, 5.8e-14, 2.7e-12),
    "masked_rkl2": (1.6e-14, 0.0e+00, 3.2e-13),
}
OTHER_CASES = {"hex27_rkl3": ("hex27_central", ("rkl", 3)), "tet10_theta0.5": ("tet10_newmark", ("theta", 0.5)),
               "rules_rkl2": ("rules_central", ("rkl", 2)), "rules_theta1": ("rules_newmark", ("theta", 1.0)),
               "masked_rkl2": ("masked_central", ("rkl", 2))}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(OTHER_CASES))
def test_other_routes_parity(engine, oracle, name):
    """Hex27 and a masked mesh and a rule-set table under RKL, Tet10 and the rule-set table under theta: the parity of the trajectory test
    (a per-element density keeps the element order: d_perm then comes from the same problem with the uniform mean density)"""
    base, case = OTHER_CASES[name]
    kind, _, asm, kw, rho = td._other_case(engine, oracle, base)
    dt = _nonlinear_dt(kind, case)
    f, lf, u0 = td._body_load(kind, td.OTHER_LOAD[kind]), td._ramp(), _shear(kind)
    tol_n = _newton_tol(td._problem(oracle, kind, "neo_hookean", f, lf, **kw), case, u0, dt)
    kwp = None
    if "rho" in kw and np.ndim(kw["rho"]) != 0:
        kwp = dict(kw)
        kwp["rho"] = float(np.mean(kw["rho"][0]))
    ref, d_perm, d_newton, tol = _measured_tolerance(oracle, kind, "neo_hookean", case, f, lf, u0, dt, 16, 4, tol_n, kw=kw or {}, kw_perm=kwp)
    tol = td._check_constants(name, d_perm, d_newton, tol, OTHER_TOLERANCE)
    ti = _integrator(case, asm, kind, dt, f, lf, newton_tol=tol_n, rho=rho)
    ti.set_state(u0)
    rec = ti.step(16, record_every=4)
    assert rec.steps_done == 16 and len(rec.time) == 4
    u, rate, _, _ = ti.state()
    _assert_parity((u, rate, _records(rec)), ref, tol, name)
    if case[0] == "rkl":   # (the element mask keeps the tiles; Hex27 and the rule-set table sum the residual first)
        assert engine.last_kernel_name() == ("k_element_pass_tiled + k_first_order_from_partials" if name == "masked_rkl2"
                                             else "k_residual_elements + k_vector_from_elements_soa + k_first_order_update")


@pytest.mark.gpu
def test_tet10_runge_kutta_legendre_is_unsupported_and_names_a_dof(engine):
    """the vertex rows of Tet10's row-sum lumped mass are not positive: decided from the value of m"""
    ti = _integrator(("rkl", 2), td._assembler(engine, "TET10", "neo_hookean"), "TET10", 1e-4)
    ti.set_state(np.zeros(3 * td._mesh("TET10")[0].num_nodes()))
    with pytest.raises(fa.FenrisError) as ei:
        ti.step(1)
    assert ei.value.code == FH_UNSUPPORTED and "dof " in ei.value.message and "not positive" in ei.value.message


# ------------------------------------------------------------------------------------------ 7. bookkeeping
@pytest.mark.gpu
@pytest.mark.parametrize("case", [("rkl", 1), ("rkl", 3), ("theta", 0.5), ("theta", 1.0)], ids=_id)
def test_records_steps_done_and_stats(engine, case):
    kind = "TET4"
    dt = _nonlinear_dt(kind, case)
    f = td._body_load(kind, 1e6)
    ti = _integrator(case, td._assembler(engine, kind, "stvk"), kind, dt, f, newton_tol=1e-11 * case[1] * dt * np.linalg.norm(f))
    ti.set_state(_shear(kind, 0.01))
    total = 0
    for every, want in ((0, [7]), (1, [1, 2, 3, 4, 5, 6, 7]), (3, [3, 6, 7]), (9, [7])):
        rec = ti.step(7, record_every=every)
        assert isinstance(rec, fa.FirstOrderRecord)
        assert rec.steps_done == 7 and rec.stats[0] == 7 and rec.stats[4] == len(want) == len(rec.time)
        assert np.allclose(rec.time, (total + np.array(want)) * dt, rtol=1e-14, atol=0.0)
        total += 7
        first = 1 if total == 7 else 0   # (the first call also forms lf_0 f - r(u_0): one more residual evaluation)
        if case[0] == "rkl":
            assert rec.stats[1] == 7 * case[1] + first and rec.stats[2] == 0 and rec.stats[3] == 0
        else:
            assert rec.stats[2] >= 7 and rec.stats[3] >= 7
            assert rec.stats[1] >= 2 * 7 + (7 if case[1] < 1.0 else 0) + first   # (Newton: the first residual and one per iteration)
        assert np.isfinite(_records(rec)).all() and (rec.mass_norm > 0).all() and (rec.stored > 0).all()
    u, rate, time, step = ti.state()
    assert step == total and abs(time - total * dt) <= 1e-14 * time and np.abs(rate).max() > 0
    with pytest.raises(fa.FenrisError) as ei:
        ti.set_state(u, np.zeros_like(u))
    assert ei.value.code == FH_BAD_ARGUMENT
    assert ti.state()[3] == total   # (the refused call left the state)


def _settings(**kw):
    s = _ffi.FirstOrderSettings()
    s.scheme, s.dt, s.stages, s.theta = _ffi.FO_THETA, 1e-3, 1, 0.5
    s.newton_tolerance, s.newton_max_iterations, s.line_search, s.preconditioner = 1e-8, 0, 1, 1
    s.linear_rel_tol, s.linear_max_iter = 1e-8, 0
    for k, v in kw.items():
        setattr(s, k, v)
    return s


@pytest.mark.gpu
def test_wrong_or_missing_settings_give_the_documented_codes(engine):
    lib = engine._lib
    asm = td._assembler(engine, "HEX8_SMALL", "stvk")
    h = C.c_void_p()

    def create(**kw):
        s = _settings(**kw)
        return lib.fh_first_order_create(engine._h, C.byref(s), C.byref(h))

    assert create() == FH_INVALID_STATE and "fh_set_mass_density" in engine.last_error()   # no density
    engine.set_mass_density(RHO)
    rkl = {"scheme": _ffi.FO_RKL}
    for kw in ({"dt": 0.0}, {"dt": -1.0}, {"dt": float("nan")}, {"dt": float("inf")}, {"scheme": 2}, {"scheme": -1}, {"theta": 0.49},
               {"theta": 1.01}, {"theta": float("nan")}, {"line_search": 7}, {"preconditioner": 9}, {"newton_tolerance": float("nan")},
               {"linear_rel_tol": float("inf")}, dict(rkl, stages=0), dict(rkl, dt=0.0), dict(rkl, dt=float("nan"))):
        assert create(**kw) == FH_BAD_ARGUMENT, kw
        assert not h.value
    assert lib.fh_first_order_create(engine._h, None, C.byref(h)) == FH_BAD_ARGUMENT
    for kind in (_ffi.MASS_VECTOR, _ffi.TENSOR):   # a mass operator, FH_TENSOR
        assert lib.fh_set_operator(engine._h, kind) == 0
        assert create() == FH_UNSUPPORTED
    assert lib.fh_set_operator(engine._h, _ffi.STVK) == 0
    assert create(**dict(rkl, theta=7.0, line_search=7)) == 0 and h.value   # (RKL reads neither theta nor the Newton arguments)
    lib.fh_dynamics_destroy(h)
    assert create() == 0 and h.value
    # fh_set_mesh invalidates the handle
    n = 3 * td._mesh("HEX8_SMALL")[0].num_nodes()
    z = np.zeros(n)
    assert lib.fh_dynamics_set_state(h, _ffi.fp(z), _ffi.fp(z)) == FH_BAD_ARGUMENT
    assert lib.fh_dynamics_set_state(h, _ffi.fp(z), None) == 0
    assert lib.fh_dynamics_step(h, 1, 0, None, None, None) == 0
    engine.set_mesh(td._mesh("HEX8_SMALL")[0])
    asm2 = td._assembler(engine, "HEX8_SMALL", "stvk")
    engine.set_mass_density(RHO)
    done = C.c_uint64(9)
    assert lib.fh_dynamics_step(h, 1, 0, None, C.byref(done), None) == FH_INVALID_STATE and done.value == 0
    assert lib.fh_dynamics_set_state(h, _ffi.fp(z), None) == FH_INVALID_STATE
    assert lib.fh_dynamics_state(h, _ffi.fp(z), None, None, None, None) == FH_INVALID_STATE
    om, dtc = C.c_double(), C.c_double()
    assert lib.fh_dynamics_stable_dt(h, 5, C.byref(om), C.byref(dtc)) == FH_INVALID_STATE
    lib.fh_dynamics_destroy(h)
    del asm, asm2


# ------------------------------------------------------------------------------------------ 8. Dirichlet entries
@pytest.mark.gpu
@pytest.mark.parametrize("case", [("rkl", 1), ("rkl", 3), ("theta", 0.5), ("theta", 1.0)], ids=_id)
def test_dirichlet_entries_come_back_bit_for_bit(engine, case):
    kind = "HEX8_SMALL"
    m = td._mesh(kind)[0]
    dt = _nonlinear_dt(kind, case)
    f = td._body_load(kind, 1e6)
    clamp = td._clamp(m)
    rng = np.random.default_rng(5)
    u0 = np.zeros_like(f)
    for k in range(3):
        u0[3 * clamp + k] = 1e-3 * rng.standard_normal(len(clamp))   # inhomogeneous values, held
    ti = _integrator(case, td._assembler(engine, kind, "neo_hookean"), kind, dt, f, newton_tol=1e-11 * case[1] * dt * np.linalg.norm(f))
    ti.set_state(u0)
    ti.step(5, record_every=2)
    u, rate, _, _ = ti.state()
    for k in range(3):
        assert np.array_equal(u[3 * clamp + k], u0[3 * clamp + k])
        assert not rate[3 * clamp + k].any()
    free = np.ones(len(f), dtype=bool)
    for k in range(3):
        free[3 * clamp + k] = False
    assert np.abs(u[free] - u0[free]).max() > 0 and np.isfinite(u).all() and np.isfinite(rate).all() and np.abs(rate[free]).max() > 0


# ------------------------------------------------------------------------------------------ 9. an inverted initial state
@pytest.mark.gpu
@pytest.mark.parametrize("case", [("rkl", 1), ("theta", 0.5), ("theta", 1.0)], ids=_id)
def test_inverted_initial_state_is_nonfinite_with_no_step_done(engine, case):
    """one Hex8 element whose u_0 flips it (x -> -x on the free face): NeoHookean puts NaN there by contract, as fh_assemble_vector does"""
    kind = "HEX8_ONE"
    x = td._mesh(kind)[0].vertices
    u0 = np.zeros(3 * len(x))
    far = np.where(np.isclose(x[:, 0], x[:, 0].max()))[0]
    u0[3 * far] = -2.0 * (x[far, 0] - x[:, 0].min())
    ti = _integrator(case, td._assembler(engine, kind, "neo_hookean"), kind, 1e-4, newton_tol=1e-10, max_it=5)
    ti.set_state(u0)
    with pytest.raises(fa.DynamicsError) as ei:
        ti.step(3)
    assert ei.value.code == FH_DYNAMICS_NONFINITE and ei.value.steps_done == 0
    assert isinstance(ei.value.record, fa.FirstOrderRecord) and len(ei.value.record.time) == 0


# ------------------------------------------------------------------------------------------ 10. stable_dt
@pytest.mark.gpu
@pytest.mark.parametrize("kind,op", [("HEX8", "elastic"), ("TET4", "elastic"), ("QUAD4", "laplace")])
def test_stable_dt(engine, oracle, kind, op):
    """omega_max^2 after 30 iterations is the reference's power iteration within the tolerance of tests/test_dynamics.py's test_stable_dt
    (the reference against its permuted self, margin 20, floor 1e-13); dt_crit = (s^2 + s) / omega_max^2 for RKL and inf for theta"""
    prob = td._problem(oracle, kind, op)
    z = np.zeros(prob.n)
    want = fr.power_iteration(prob, z, 30)
    d_perm = abs(fr.power_iteration(td._problem(oracle, kind, op, perm=7), z, 30) - want) / want
    tol = td._check_constants((kind, op), d_perm, 0.0, max(20.0 * d_perm, 1e-13), td.STABLE_DT_TOLERANCE)
    asm = td._assembler(engine, kind, op)
    for case in (("rkl", 1), ("rkl", 6), ("theta", 0.5)):
        ti = _integrator(case, asm, kind, 1e-3)
        ti.set_state(z)
        om, dtc = ti.stable_dt(30)
        print(f"{kind} {op} {_id(case)}: omega_max^2 {om * om:.6e}, reference {want:.6e}, dt_crit {dtc:.6e}")
        assert abs(om * om - want) <= tol * want
        if case[0] == "rkl":
            s = case[1]
            assert dtc == (s * s + s) / (om * om)
        else:
            assert dtc == float("inf")
        ti.close()


# ------------------------------------------------------------------------------------------ 11. repeatability
def _run_cut(engine, case, cut, device=False):
    """12 steps: "one": a single call with a record every 4 (steps 4, 8, 12); "two": 5 steps with a record every 4 (steps 4, 5), then 7
    with a record every 3 (steps 8, 11, 12).  Returns u and the record rows of steps 4, 8 and 12"""
    kind = "HEX8"
    dt = _nonlinear_dt(kind, case)
    f, lf, u0 = td._body_load(kind, td.LOAD[kind]), td._ramp(), _shear(kind)
    ti = _integrator(case, td._assembler(engine, kind, "neo_hookean"), kind, dt, f, lf, newton_tol=1e-9 * case[1] * dt * np.linalg.norm(f))
    if device:
        import torch

        ti.with_load(torch.from_numpy(f).to("cuda:0"), lf)
        ti.set_state(torch.from_numpy(u0).to("cuda:0"))
    else:
        ti.set_state(u0)
    if cut == "one":
        rows = _records(ti.step(12, record_every=4))
    else:
        a, b = _records(ti.step(5, record_every=4)), _records(ti.step(7, record_every=3))
        rows = np.stack([a[0], b[0], b[2]])
    u, rate, time, step = ti.state(device=device)
    if device:
        u, rate = u.cpu().numpy(), rate.cpu().numpy()
    assert step == 12 and rows.shape == (3, 4)
    ti.close()
    return u, rate, rows, time


@pytest.mark.gpu
@pytest.mark.parametrize("case", [("rkl", 1), ("rkl", 3), ("theta", 0.5)], ids=_id)
def test_runs_repeat_and_restart_bit_for_bit(engine, case):
    """12 steps in one call, the same as 5 + 7 with other record cadences, the same in a second engine and through the _dev entry points:
    identical bits in u, the rate and the record rows of the common steps"""
    base = _run_cut(engine, case, "one")
    assert np.isfinite(base[0]).all() and np.abs(base[0]).max() > 0 and np.allclose(base[2][:, 3] / base[2][0, 3], [1.0, 2.0, 3.0])
    second = fa.Engine(0)
    try:
        for eng, cut, device in ((engine, "two", False), (second, "one", False), (second, "two", True), (engine, "one", True)):
            other = _run_cut(eng, case, cut, device)
            for name, p, q in zip(("u", "rate", "records", "time"), base, other):
                assert np.array_equal(np.asarray(p), np.asarray(q)), (_id(case), cut, device, name)
    finally:
        second.close()
