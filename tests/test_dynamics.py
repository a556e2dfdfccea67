"""Device-resident time integration (fh_dynamics_*, fenris_amd.dynamics): central differences, Newmark and backward Euler against the
NumPy statement of tests/dynamics_reference.py, which is pinned here on the CPU against the closed forms of a single eigenmode."""
import functools
import os

import numpy as np
import pytest

import fenris_amd as fa
from fenris_amd import _ffi, quadrature

import dynamics_reference as dr

LAME = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.3))
RHO = 1000.0
FH_BAD_ARGUMENT, FH_INVALID_STATE, FH_UNSUPPORTED, FH_DYNAMICS_NONFINITE = 2, 5, 6, 15
OKIND = {"QUAD4": 0, "HEX8": 1, "TET4": 2, "HEX27": 3, "TRI3": 4, "TET10": 5, "QUAD9": 6}
SCHEMES = ("central", "newmark", "euler")
NEW = ("fh_dynamics_create", "fh_dynamics_destroy", "fh_dynamics_set_state", "fh_dynamics_set_state_dev", "fh_dynamics_set_load",
       "fh_dynamics_set_load_dev", "fh_dynamics_step", "fh_dynamics_state", "fh_dynamics_state_dev", "fh_dynamics_stable_dt")


@pytest.fixture()
def engine():
    eng = fa.Engine(0)
    yield eng
    eng.close()


# ------------------------------------------------------------------------------------------ meshes, problems, integrators
@functools.lru_cache(maxsize=None)
def _mesh(kind):
    """the smallest shapes with a ragged second tile and a ragged second node workgroup (Hex8 288 elements / 441 nodes, Tet4 324 / 91,
    Quad4 400 / 441, Tri3 of the same square), and small quadratic meshes for the routes off the tiles"""
    P, T, Q = fa.procedural, quadrature.tensor, quadrature.total_order
    make = {"HEX8": (lambda: P.create_rectangular_uniform_hex_mesh(1.0, 8, 6, 6, 1), T.hexahedron_gauss(2)),
            "TET4": (lambda: P.create_unit_box_uniform_tet_mesh_3d(3), Q.tetrahedron(2)),
            "QUAD4": (lambda: P.create_unit_square_uniform_quad_mesh_2d(20), T.quadrilateral_gauss(2)),
            "TRI3": (lambda: P.create_unit_square_uniform_tri_mesh_2d(20), Q.triangle(2)),
            "HEX27": (lambda: fa.hex27_mesh_from_hex8(P.create_unit_box_uniform_hex_mesh_3d(2)), T.hexahedron_gauss(3)),
            "TET10": (lambda: fa.tet10_mesh_from_tet4(P.create_unit_box_uniform_tet_mesh_3d(2)), Q.tetrahedron(4)),
            "QUAD9": (lambda: fa.quad9_mesh_from_quad4(P.create_unit_square_uniform_quad_mesh_2d(4)), T.quadrilateral_gauss(3)),
            "HEX8_ONE": (lambda: P.create_unit_box_uniform_hex_mesh_3d(1), T.hexahedron_gauss(2)),
            "HEX8_SMALL": (lambda: P.create_unit_box_uniform_hex_mesh_3d(2), T.hexahedron_gauss(2)),
            "HEX8_MID": (lambda: P.create_unit_box_uniform_hex_mesh_3d(3), T.hexahedron_gauss(2)),
            "TET4_SMALL": (lambda: P.create_unit_box_uniform_tet_mesh_3d(2), Q.tetrahedron(2)),
            "QUAD4_SMALL": (lambda: P.create_unit_square_uniform_quad_mesh_2d(6), T.quadrilateral_gauss(2))}
    gen, (w, p) = make[kind]
    return gen(), np.asarray(w), np.asarray(p)


def _okind(kind):
    return OKIND[kind.split("_")[0]]


def _oop(oracle, op):
    return {"laplace": oracle.LAPLACE, "elastic": oracle.LINEAR_ELASTIC, "neo_hookean": oracle.NEO_HOOKEAN, "stvk": oracle.STVK}[op]


def _clamp(m):
    x = m.vertices[:, 0]
    return np.where(np.isclose(x, x.min()))[0]


def _problem(oracle, kind, op, f=None, load_factor=None, groups=None, rho=RHO, direct="dense", perm=None):
    """the reference's problem; perm: a permutation of the connectivity rows (another summation order in r, nothing else)"""
    m, w, p = _mesh(kind)
    if groups is None:
        groups = [(np.asarray(m.connectivity), w, p)]
    if perm is not None:
        groups = [(c[np.random.default_rng(perm + g).permutation(len(c))], wg, pg) for g, (c, wg, pg) in enumerate(groups)]
        assert np.ndim(rho) == 0
    return dr.Problem(oracle, _okind(kind), _oop(oracle, op), m.vertices, groups, params=None if op == "laplace" else LAME.as_pair(), rho=rho,
                      dirichlet=_clamp(m), f=f, load_factor=load_factor, direct=direct)


def _operator(op):
    return {"laplace": fa.LaplaceOperator(), "elastic": fa.MaterialEllipticOperator(fa.LinearElasticMaterial()),
            "neo_hookean": fa.MaterialEllipticOperator(fa.NeoHookeanMaterial()), "stvk": fa.MaterialEllipticOperator(fa.StVKMaterial())}[op]


def _assembler(engine, kind, op, qt=None):
    m, w, p = _mesh(kind)
    s = 1 if op == "laplace" else m.vertices.shape[1]
    if qt is None:
        qt = fa.UniformQuadratureTable.from_points_and_weights(p, w)
        qt = qt if op == "laplace" else qt.with_uniform_data(LAME)
    return (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(m).with_operator(_operator(op)).with_quadrature_table(qt)
            .with_u(np.zeros(s * m.num_nodes())).build())


def _integrator(scheme, asm, kind, dt, f=None, load_factor=None, newton_tol=1e-8, max_it=None, rho=RHO):
    clamp = _clamp(_mesh(kind)[0])
    if scheme == "central":
        ti = fa.CentralDifference(asm, rho, dt)
    else:
        ti = fa.Newmark(asm, rho, dt) if scheme == "newmark" else fa.BackwardEuler(asm, rho, dt)
        ti.with_newton(fa.NewtonSettings(max_it, newton_tol), linear_rel_tol=1e-12)
    return ti.with_dirichlet_nodes(clamp).with_load(f, load_factor)


@functools.lru_cache(maxsize=None)
def _modal(kind, op):
    """dense pencils of the clamped body at u = 0: dt = 0.5 * 2 / omega_max of (K, diag m), the lowest two modes of (K, diag m) and of
    (K, M), and the condition numbers of M + beta dt^2 K on the free dofs for beta = 1/4 and 1"""
    from oracle import oracle as o

    o.lib()
    prob = _problem(o, kind, op)
    z = np.zeros(prob.n)
    wc, Vc = dr.dense_pencil(prob, z, False)
    lumped_ok = (prob.lumped()[prob.free] > 0).all()   # (Tet10: no lumped pencil; dt then comes from the consistent one)
    wl, Vl = dr.dense_pencil(prob, z, True) if lumped_ok else (wc, Vc)
    dt = 0.5 * 2.0 / np.sqrt(wl[-1])
    fr = prob.free
    K, M = prob.tangent(z)[fr][:, fr].toarray(), prob.mass()[fr][:, fr].toarray()
    kappa = {"newmark": np.linalg.cond(M + 0.25 * dt * dt * K), "euler": np.linalg.cond(M + dt * dt * K)}
    return {"dt": dt, "lam_max": wl[-1], "central": (np.sqrt(wl[:2]), Vl[:, :2]), "newmark": (np.sqrt(wc[:2]), Vc[:, :2]),
            "euler": (np.sqrt(wc[:2]), Vc[:, :2]), "kappa": kappa, "Kphi": np.linalg.norm(prob.tangent(z) @ Vc[:, 0])}


def _reference_run(prob, scheme, u0, v0, dt, steps, record_every, tol=1e-8):
    if scheme == "central":
        u, v, a, rec = dr.central_difference(prob, u0, v0, dt, steps, record_every)
        return u, v, a, rec
    st, u, v, a, rec, done, _ = dr.implicit(prob, scheme, u0, v0, dt, steps, record_every, tol=tol)
    assert st == "ok" and done == steps
    return u, v, a, rec


def _rel_diff(x, y):
    """the largest difference over (u, v, a, every record column), each relative to the first trajectory's largest magnitude"""
    out = 0.0
    for p, q in zip(x[:3], y[:3]):
        out = max(out, np.abs(p - q).max() / max(np.abs(p).max(), 1e-300))
    for c in range(4):
        out = max(out, np.abs(x[3][:, c] - y[3][:, c]).max() / max(np.abs(x[3][:, c]).max(), 1e-300))
    return out


def _measured_tolerance(oracle, kind, op, scheme, f, lf, dt, steps, every, tol, **kw):
    """the reference against itself: d_perm from a permuted connectivity (another summation order in r), d_newton from a Newton tolerance
    100 times smaller; the device differs from the oracle in summation order in every residual and reduction, each an independent
    rounding difference of the size d_perm samples once, hence 20 (d_perm + d_newton), and never below 1e-13"""
    n = _problem(oracle, kind, op).n
    z = np.zeros(n)
    ref = _reference_run(_problem(oracle, kind, op, f, lf, **kw), scheme, z, z, dt, steps, every, tol)
    perm = _reference_run(_problem(oracle, kind, op, f, lf, perm=7, **kw), scheme, z, z, dt, steps, every, tol)
    d_perm = _rel_diff(ref, perm)
    d_newton = 0.0
    if scheme != "central":
        d_newton = _rel_diff(ref, _reference_run(_problem(oracle, kind, op, f, lf, **kw), scheme, z, z, dt, steps, every, tol / 100.0))
    return ref, d_perm, d_newton, max(20.0 * (d_perm + d_newton), 1e-13)


def _assert_parity(got, ref, tol, what=""):
    for name, p, q in zip("uva", got[:3], ref[:3]):
        err = np.abs(p - q).max() / max(np.abs(q).max(), 1e-300)
        print(f"{what} {name}: {err:.3e} (tol {tol:.3e})")
        assert err <= tol, (what, name, err, tol)
    for c, name in enumerate(("kinetic", "stored", "load_potential", "time")):
        err = np.abs(got[3][:, c] - ref[3][:, c]).max() / max(np.abs(ref[3][:, c]).max(), 1e-300)
        print(f"{what} {name}: {err:.3e} (tol {tol:.3e})")
        assert err <= tol, (what, name, err, tol)


def _records(rec):
    return np.stack([rec.kinetic, rec.stored, rec.load_potential, rec.time], axis=1)


def _body_load(kind, total):
    """a force `total` along +x spread evenly over all nodes (the clamped ones take none)"""
    m = _mesh(kind)[0]
    d = m.vertices.shape[1]
    f = np.zeros(d * m.num_nodes())
    f[0::d] = total / m.num_nodes()
    f[d * _clamp(m)] = 0.0
    return f


# ------------------------------------------------------------------------------------------ no GPU: declarations, the reference pinned
def test_dynamics_entry_points_are_declared():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fenris_hip.h")).read()
    for name in NEW:
        assert name in _ffi.exported_symbols() and name + "(" in hdr
    for text in ("FH_DYNAMICS_NONFINITE = 15", "FH_DYN_CENTRAL_DIFFERENCE = 0, FH_DYN_BACKWARD_EULER = 1, FH_DYN_NEWMARK = 2", "} fh_dynamics_settings;",
                 "#define FH_ABI_VERSION 1"):
        assert text in hdr
    assert issubclass(fa.DynamicsError, fa.FenrisError)
    for cls in (fa.CentralDifference, fa.Newmark, fa.BackwardEuler):
        assert issubclass(cls, fa.TimeIntegrator)
    assert _ffi.FH_DYNAMICS_NONFINITE == 15 and (_ffi.DYN_CENTRAL_DIFFERENCE, _ffi.DYN_BACKWARD_EULER, _ffi.DYN_NEWMARK) == (0, 1, 2)


def test_reference_reproduces_the_start_vector():
    """column 0 of fh_eigs_lowest's fill, against splitmix64 in Python integers"""
    def sm(z):
        mask = (1 << 64) - 1
        z = (z + 0x9E3779B97F4A7C15) & mask
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
        return z ^ (z >> 31)

    x = dr.splitmix_column0(300)
    want = np.array([(sm(i) >> 11) * 2.0 ** -52 - 1.0 for i in range(300)])
    assert np.array_equal(x, want) and x.min() >= -1.0 and x.max() < 1.0 and abs(x.mean()) < 0.2


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("kind,op", [("HEX8_SMALL", "elastic"), ("TET4_SMALL", "elastic"), ("QUAD4_SMALL", "laplace")])
def test_reference_meets_the_closed_forms(oracle, kind, op, scheme):
    """u_0 = phi, v_0 = 0, f = 0 on one eigenmode of the scheme's dense pencil: u_n = c_n phi to 1e-10 max|phi| over 32 steps (dense solves
    leave only rounding)"""
    md = _modal(kind, op)
    om, V = md[scheme]
    phi, dt = V[:, 0], md["dt"]
    prob = _problem(oracle, kind, op)
    for n in (1, 2, 7, 32):
        u = _reference_run(prob, scheme, phi, np.zeros_like(phi), dt, n, 0, tol=1e-12 * md["Kphi"])[0]
        assert np.abs(u - dr.closed_form(scheme, om[0], dt, n) * phi).max() <= 1e-10 * np.abs(phi).max()


def test_reference_mass_with_element_densities(oracle):
    """the per-element density of the reference's mass: the sum of one-element problems"""
    m, w, p = _mesh("HEX8_SMALL")
    conn = np.asarray(m.connectivity)
    rho = np.linspace(500.0, 1500.0, len(conn))
    M = _problem(oracle, "HEX8_SMALL", "elastic", rho=[rho]).mass().toarray()
    want = sum(_problem(oracle, "HEX8_SMALL", "elastic", groups=[(conn[e:e + 1], w, p)], rho=float(rho[e])).mass().toarray() for e in range(len(conn)))
    assert np.abs(M - want).max() <= 1e-13 * np.abs(want).max()


# ------------------------------------------------------------------------------------------ 1. single-mode closed forms on the device
@pytest.mark.gpu
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("kind,op", [("HEX8", "elastic"), ("TET4", "elastic"), ("QUAD4", "laplace")])
def test_single_mode_closed_forms(engine, kind, op, scheme):
    """32 steps on one eigenmode.  Central differences involve rounding only (neutrally stable: steps^2 times a few ulp), 1e-10 max|phi|;
    the implicit schemes solve to linear_rel_tol = 1e-12, so 10 steps kappa linear_rel_tol max|phi| with kappa of M + beta dt^2 K"""
    md = _modal(kind, op)
    om, V = md[scheme]
    phi, dt, steps = V[:, 0], md["dt"], 32
    tol = 1e-10 if scheme == "central" else 10.0 * steps * md["kappa"][scheme] * 1e-12
    ti = _integrator(scheme, _assembler(engine, kind, op), kind, dt, newton_tol=1e-12 * md["Kphi"])
    ti.set_state(phi)
    worst = 0.0
    for n in range(1, steps + 1):
        rec = ti.step(1)
        assert rec.steps_done == 1 and len(rec.time) == 1 and abs(rec.time[0] - n * dt) <= 1e-14 * n * dt
        u = ti.state()[0]
        worst = max(worst, np.abs(u - dr.closed_form(scheme, om[0], dt, n) * phi).max() / np.abs(phi).max())
    print(f"{kind} {op} {scheme}: worst error {worst:.3e} of max|phi| (tol {tol:.3e})")
    assert worst <= tol


# ------------------------------------------------------------------------------------------ 2. exact invariants, linear operators
@pytest.mark.gpu
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("kind,op", [("HEX8", "elastic"), ("TET4", "elastic"), ("QUAD4", "laplace"), ("TRI3", "laplace")])
def test_invariants_of_the_linear_schemes(engine, oracle, kind, op, scheme):
    """f = 0, 64 steps from u_0 = phi_0, v_0 = omega_1 phi_1 / 2.  Central differences conserve 1/2 v^T m v + 1/2 u^T K u - dt^2/8 a^T m a
    (relative drift <= 1e-11); Newmark (1/4, 1/2) conserves kinetic + stored and backward Euler's never increases, both within
    10 steps kappa linear_rel_tol"""
    md = _modal(kind, op)
    om, V = md[scheme]
    dt, steps = md["dt"], 64
    u0, v0 = V[:, 0], 0.5 * om[1] * V[:, 1]
    ti = _integrator(scheme, _assembler(engine, kind, op), kind, dt, newton_tol=1e-12 * md["Kphi"])
    ti.set_state(u0, v0)
    prob = _problem(oracle, kind, op)
    m = prob.lumped()
    E0 = 0.5 * float(v0 @ ((m * v0) if scheme == "central" else (prob.mass() @ v0))) + prob.energy(u0)
    if scheme == "central":
        a0 = ti.state()[2]
        H = [E0 - dt * dt / 8.0 * float(np.sum(m * a0 * a0))]
        for _ in range(8):
            rec = ti.step(8)
            a = ti.state()[2]
            H.append(rec.kinetic[-1] + rec.stored[-1] - dt * dt / 8.0 * float(np.sum(m * a * a)))
        drift = np.abs(np.array(H) - H[0]).max() / abs(H[0])
        print(f"{kind} {op} central: relative drift of the invariant {drift:.3e}")
        assert drift <= 1e-11
        return
    rec = ti.step(steps, record_every=1)
    assert len(rec.time) == steps
    E = np.concatenate([[E0], rec.kinetic + rec.stored])
    bound = 10.0 * steps * md["kappa"][scheme] * 1e-12
    if scheme == "newmark":
        drift = np.abs(E - E[0]).max() / E[0]
        print(f"{kind} {op} newmark: relative energy drift {drift:.3e} (bound {bound:.3e})")
        assert drift <= bound
    else:
        rise = np.max(np.diff(E)) / E[0]
        print(f"{kind} {op} euler: largest relative energy rise {rise:.3e} (bound {bound:.3e}), E_64 / E_0 = {E[-1] / E[0]:.4f}")
        assert rise <= bound and E[-1] < E[0]


# ------------------------------------------------------------------------------------------ 3. trajectory parity, nonlinear
# The load: a ramp over the first 8 steps, then held, spread over all nodes along +x and sized on the CPU reference so that the peak
# displacement of the 16 steps is about 10 % of the body's length along x.
LOAD = {"HEX8": 1.0e7, "TET4": 1.4e5}
# Measured on the CPU with the reference alone (_measured_tolerance): d_perm, d_newton and the resulting tolerance 20 (d_perm + d_newton),
# floored at 1e-13, per (mesh, material, scheme).  The test measures them again and asserts that they stay within a factor 10 of these.
TRAJECTORY_TOLERANCE = {
    ("HEX8", "neo_hookean", "central"): (2.4e-14, 0.0e+00, 4.8e-13),
    ("HEX8", "neo_hookean", "newmark"): (1.2e-13, 2.8e-12, 5.9e-11),
    ("HEX8", "neo_hookean", "euler"): (2.9e-14, 1.4e-11, 2.8e-10),
    ("HEX8", "stvk", "central"): (2.7e-14, 0.0e+00, 5.3e-13),
    ("HEX8", "stvk", "newmark"): (1.2e-13, 1.7e-10, 3.3e-09),
    ("HEX8", "stvk", "euler"): (3.1e-14, 0.0e+00, 6.3e-13),
    ("TET4", "neo_hookean", "central"): (2.9e-14, 0.0e+00, 5.7e-13),
    ("TET4", "neo_hookean", "newmark"): (1.0e-13, 1.7e-12, 3.5e-11),
    ("TET4", "neo_hookean", "euler"): (4.1e-14, 7.3e-11, 1.5e-09),
    ("TET4", "stvk", "central"): (2.4e-14, 0.0e+00, 4.8e-13),
    ("TET4", "stvk", "newmark"): (8.5e-14, 1.1e-11, 2.1e-10),
    ("TET4", "stvk", "euler"): (3.1e-14, 0.0e+00, 6.2e-13),
}


def _ramp():
    return np.linspace(0.0, 1.0, 8)


def _newton_tol(f, dt, scheme):
    """1e-11 ||beta dt^2 f||: both the reference and the device then stop at rounding level, some orders above the floor of F"""
    return 1e-11 * np.linalg.norm(f) * {"central": 0.0, "newmark": 0.25, "euler": 1.0}[scheme] * dt * dt


def _check_constants(key, d_perm, d_newton, tol, table):
    c_perm, c_newton, c_tol = table[key]
    print(f"{key}: d_perm {d_perm:.3e} (constant {c_perm:.3e}), d_newton {d_newton:.3e} ({c_newton:.3e}), tolerance {tol:.3e} ({c_tol:.3e})")
    assert c_tol / 10.0 <= tol <= 10.0 * c_tol, (key, d_perm, d_newton, tol)
    return c_tol


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("op", ["neo_hookean", "stvk"])
@pytest.mark.parametrize("kind", ["HEX8", "TET4"])
def test_trajectory_parity_with_the_reference(engine, oracle, kind, op, scheme):
    """16 steps under the ramped load with a record every 4: u, v, a and every record row against the reference"""
    dt = _modal(kind, "elastic")["dt"]
    f, lf = _body_load(kind, LOAD[kind]), _ramp()
    tol_n = _newton_tol(f, dt, scheme)
    ref, d_perm, d_newton, tol = _measured_tolerance(oracle, kind, op, scheme, f, lf, dt, 16, 4, tol_n, direct="sparse")
    tol = _check_constants((kind, op, scheme), d_perm, d_newton, tol, TRAJECTORY_TOLERANCE)
    ti = _integrator(scheme, _assembler(engine, kind, op), kind, dt, f, lf, newton_tol=tol_n)
    ti.set_state(np.zeros_like(f))
    rec = ti.step(16, record_every=4)
    assert rec.steps_done == 16 and len(rec.time) == 4 and rec.stats[0] == 16 and rec.stats[4] == 4
    u, v, a, time, step = ti.state()
    assert step == 16 and abs(time - 16 * dt) <= 1e-14 * time
    _assert_parity((u, v, a, _records(rec)), ref, tol, f"{kind} {op} {scheme}")
    d = _mesh(kind)[0].vertices.shape[1]
    x = _mesh(kind)[0].vertices[:, 0]
    peak = np.abs(u).max() / (x.max() - x.min())
    print(f"{kind} {op} {scheme}: peak displacement {peak:.3f} of the body's length")
    assert 0.03 <= peak <= 0.3 and d == 3


# ------------------------------------------------------------------------------------------ 4. the other routes
OTHER_LOAD = {"HEX27": 1.1e5, "TET10": 3.8e5, "HEX8_SMALL": 1.3e5, "HEX8_MID": 1.3e5}
# measured like TRAJECTORY_TOLERANCE, per case
OTHER_TOLERANCE = {
    "hex27_central": (5.3e-14, 0.0e+00, 1.1e-12),
    "tet10_newmark": (2.2e-14, 0.0e+00, 4.4e-13),
    "rules_newmark": (4.6e-14, 7.7e-12, 1.5e-10),
    "rules_central": (7.3e-15, 0.0e+00, 1.5e-13),
    "masked_central": (1.6e-14, 0.0e+00, 3.3e-13),
}


def _other_case(engine, oracle, case):
    """(kind, scheme, assembler, reference keywords, density of the device): Hex27 central differences; Tet10 Newmark; a Hex8 rule-set table
    under Newmark and central differences; a masked Hex8 mesh with a per-element density"""
    if case == "hex27_central":
        return "HEX27", "central", _assembler(engine, "HEX27", "neo_hookean"), {}, RHO
    if case == "tet10_newmark":
        return "TET10", "newmark", _assembler(engine, "TET10", "neo_hookean"), {}, RHO
    m, w, p = _mesh("HEX8_SMALL")
    conn = np.asarray(m.connectivity)
    E = len(conn)
    if case.startswith("rules"):
        w2, p2 = (np.asarray(a) for a in quadrature.tensor.hexahedron_gauss(3))
        emap = (np.arange(E) % 2).astype(np.uint64)
        qt = fa.compact_quadrature_table([p, p2], [w, w2], [[LAME] * len(w), [LAME] * len(w2)], emap)
        groups = [(conn[emap == 0], w, p), (conn[emap == 1], w2, p2)]
        return "HEX8_SMALL", case.split("_")[1], _assembler(engine, "HEX8_SMALL", "neo_hookean", qt=qt), {"groups": groups}, RHO
    m, w, p = _mesh("HEX8_MID")   # masked_central: the centre element of a 3 x 3 x 3 box is inactive (every node keeps an active element)
    conn = np.asarray(m.connectivity)
    E = len(conn)
    mask = np.ones(E, dtype=np.uint8)
    mask[np.argmin(np.abs(m.vertices[conn.astype(np.int64)].mean(axis=1) - 0.5).sum(axis=1))] = 0
    rho = np.linspace(800.0, 1200.0, E)
    asm = _assembler(engine, "HEX8_MID", "neo_hookean")
    engine.set_active_elements(mask)
    return "HEX8_MID", "central", asm, {"groups": [(conn[mask == 1], w, p)], "rho": [rho[mask == 1]]}, rho


def _measured_other(oracle, kind, scheme, f, lf, dt, tol_n, kw):
    """_measured_tolerance for a problem given by keywords (a per-element density keeps the element order: d_perm then comes from the
    same problem with the uniform mean density, which samples the same rounding)"""
    z = np.zeros(len(f))
    ref = _reference_run(_problem(oracle, kind, "neo_hookean", f, lf, **kw), scheme, z, z, dt, 16, 4, tol_n)
    kwp = dict(kw)
    if "rho" in kwp and np.ndim(kwp["rho"]) != 0:
        kwp["rho"] = float(np.mean(kwp["rho"][0]))
    base = _reference_run(_problem(oracle, kind, "neo_hookean", f, lf, **kwp), scheme, z, z, dt, 16, 4, tol_n)
    perm = _reference_run(_problem(oracle, kind, "neo_hookean", f, lf, perm=7, **kwp), scheme, z, z, dt, 16, 4, tol_n)
    d_perm = _rel_diff(base, perm)
    d_newton = 0.0
    if scheme != "central":
        d_newton = _rel_diff(ref, _reference_run(_problem(oracle, kind, "neo_hookean", f, lf, **kw), scheme, z, z, dt, 16, 4, tol_n / 100.0))
    return ref, d_perm, d_newton, max(20.0 * (d_perm + d_newton), 1e-13)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["hex27_central", "tet10_newmark", "rules_newmark", "rules_central", "masked_central"])
def test_other_routes_parity(engine, oracle, case):
    kind, scheme, asm, kw, rho = _other_case(engine, oracle, case)
    dt = _modal(kind, "elastic")["dt"]
    f, lf = _body_load(kind, OTHER_LOAD[kind]), _ramp()
    tol_n = _newton_tol(f, dt, scheme)
    ref, d_perm, d_newton, tol = _measured_other(oracle, kind, scheme, f, lf, dt, tol_n, kw)
    tol = _check_constants(case, d_perm, d_newton, tol, OTHER_TOLERANCE)
    ti = _integrator(scheme, asm, kind, dt, f, lf, newton_tol=tol_n, rho=rho)
    ti.set_state(np.zeros_like(f))
    rec = ti.step(16, record_every=4)
    assert rec.steps_done == 16 and len(rec.time) == 4
    u, v, a, _, _ = ti.state()
    _assert_parity((u, v, a, _records(rec)), ref, tol, case)
    if scheme == "central":   # the name of the step's launch, read before a record's energy pass replaces it: a_0 of a second integrator
        ti.close()
        t2 = _integrator(scheme, asm, kind, dt, f, lf, newton_tol=tol_n, rho=rho)
        t2.set_state(np.zeros_like(f))
        t2.state()
        assert engine.last_kernel_name() == ("k_element_pass_tiled + k_dynamics_from_partials" if case == "masked_central"
                                             else "k_residual_elements + k_vector_from_elements_soa + k_dynamics_update"), engine.last_kernel_name()
        t2.close()


@pytest.mark.gpu
def test_tet10_central_difference_is_unsupported_and_names_a_dof(engine):
    """the vertex rows of Tet10's row-sum lumped mass are not positive: decided from the value of m"""
    ti = _integrator("central", _assembler(engine, "TET10", "neo_hookean"), "TET10", 1e-4)
    ti.set_state(np.zeros(3 * _mesh("TET10")[0].num_nodes()))
    with pytest.raises(fa.FenrisError) as ei:
        ti.step(1)
    assert ei.value.code == FH_UNSUPPORTED and "dof " in ei.value.message and "not positive" in ei.value.message


# ------------------------------------------------------------------------------------------ 5. contract
@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["central", "newmark"])
def test_records_steps_done_and_stats(engine, scheme):
    kind = "TET4"
    dt = _modal(kind, "elastic")["dt"]
    f = _body_load(kind, 1e6)
    ti = _integrator(scheme, _assembler(engine, kind, "stvk"), kind, dt, f, newton_tol=_newton_tol(f, dt, scheme))
    ti.set_state(np.zeros_like(f))
    total = 0
    for every, want in ((0, [7]), (1, [1, 2, 3, 4, 5, 6, 7]), (3, [3, 6, 7]), (9, [7])):
        rec = ti.step(7, record_every=every)
        assert rec.steps_done == 7 and rec.stats[0] == 7 and rec.stats[4] == len(want) == len(rec.time)
        assert np.allclose(rec.time, (total + np.array(want)) * dt, rtol=1e-14, atol=0.0)
        total += 7
        first = 1 if total == 7 else 0   # (the first call also forms a_0: one more residual evaluation, and for Newmark one PCG solve)
        if scheme == "central":
            assert rec.stats[1] == 7 + first and rec.stats[2] == 0 and rec.stats[3] == 0
        else:
            assert rec.stats[2] >= 7 and rec.stats[1] >= 14 + first and rec.stats[3] >= 7
        assert np.isfinite(rec.kinetic).all() and (rec.kinetic > 0).all() and (rec.stored > 0).all() and (rec.load_potential > 0).all()
    assert ti.state()[4] == total


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", SCHEMES)
def test_dirichlet_entries_come_back_bit_for_bit(engine, scheme):
    kind = "HEX8_SMALL"
    m = _mesh(kind)[0]
    dt = _modal(kind, "elastic")["dt"]
    f = _body_load(kind, 1e6)
    clamp = _clamp(m)
    rng = np.random.default_rng(5)
    u0, v0 = np.zeros_like(f), 1e-3 * rng.standard_normal(len(f))
    for k in range(3):
        u0[3 * clamp + k] = 1e-3 * rng.standard_normal(len(clamp))   # inhomogeneous values, held
    ti = _integrator(scheme, _assembler(engine, kind, "neo_hookean"), kind, dt, f, newton_tol=_newton_tol(f, dt, scheme))
    ti.set_state(u0, v0)
    ti.step(5, record_every=2)
    u, v, a, _, _ = ti.state()
    for k in range(3):
        assert np.array_equal(u[3 * clamp + k], u0[3 * clamp + k])
        assert not v[3 * clamp + k].any() and not a[3 * clamp + k].any()
    free = np.ones(len(f), dtype=bool)
    for k in range(3):
        free[3 * clamp + k] = False
    assert np.abs(u[free] - u0[free]).max() > 0 and np.isfinite(u).all()


def _settings(**kw):
    s = _ffi.DynamicsSettings()
    s.scheme, s.dt, s.newmark_beta, s.newmark_gamma = _ffi.DYN_NEWMARK, 1e-3, 0.25, 0.5
    s.newton_tolerance, s.newton_max_iterations, s.line_search, s.preconditioner = 1e-8, 0, 1, 1
    s.linear_rel_tol, s.linear_max_iter = 1e-8, 0
    for k, v in kw.items():
        setattr(s, k, v)
    return s


@pytest.mark.gpu
def test_wrong_or_missing_settings_give_the_documented_codes(engine):
    import ctypes as C

    lib = engine._lib
    asm = _assembler(engine, "HEX8_SMALL", "stvk")
    h = C.c_void_p()

    def create(**kw):
        s = _settings(**kw)
        return lib.fh_dynamics_create(engine._h, C.byref(s), C.byref(h))

    assert create() == FH_INVALID_STATE and "fh_set_mass_density" in engine.last_error()   # no density
    engine.set_mass_density(RHO)
    for kw in ({"dt": 0.0}, {"dt": -1.0}, {"dt": float("nan")}, {"newmark_beta": 0.0}, {"newmark_beta": -0.25}, {"scheme": 3}, {"scheme": -1},
               {"newmark_gamma": float("inf")}, {"line_search": 7}, {"preconditioner": 9}, {"newton_tolerance": float("nan")}):
        assert create(**kw) == FH_BAD_ARGUMENT, kw
        assert not h.value
    assert lib.fh_dynamics_create(engine._h, None, C.byref(h)) == FH_BAD_ARGUMENT
    for kind in (_ffi.MASS_VECTOR, _ffi.TENSOR):   # a mass operator, FH_TENSOR
        assert lib.fh_set_operator(engine._h, kind) == 0
        assert create() == FH_UNSUPPORTED
    assert lib.fh_set_operator(engine._h, _ffi.STVK) == 0
    assert create() == 0 and h.value
    # fh_set_mesh invalidates the handle
    n = 3 * _mesh("HEX8_SMALL")[0].num_nodes()
    z = np.zeros(n)
    assert lib.fh_dynamics_set_state(h, _ffi.fp(z), None) == 0
    assert lib.fh_dynamics_step(h, 1, 0, None, None, None) == 0
    engine.set_mesh(_mesh("HEX8_SMALL")[0])
    asm2 = _assembler(engine, "HEX8_SMALL", "stvk")
    engine.set_mass_density(RHO)
    done = C.c_uint64(9)
    assert lib.fh_dynamics_step(h, 1, 0, None, C.byref(done), None) == FH_INVALID_STATE and done.value == 0
    assert lib.fh_dynamics_set_state(h, _ffi.fp(z), None) == FH_INVALID_STATE
    assert lib.fh_dynamics_state(h, _ffi.fp(z), None, None, None, None) == FH_INVALID_STATE
    om, dtc = C.c_double(), C.c_double()
    assert lib.fh_dynamics_stable_dt(h, 5, C.byref(om), C.byref(dtc)) == FH_INVALID_STATE
    lib.fh_dynamics_destroy(h)
    del asm, asm2


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", SCHEMES)
def test_inverted_initial_state_is_nonfinite_with_no_step_done(engine, scheme):
    """one Hex8 element whose u_0 flips it (x -> -x on the free face): NeoHookean puts NaN there by contract, as fh_assemble_vector does"""
    kind = "HEX8_ONE"
    m = _mesh(kind)[0]
    x = m.vertices
    u0 = np.zeros(3 * len(x))
    far = np.where(np.isclose(x[:, 0], x[:, 0].max()))[0]
    u0[3 * far] = -2.0 * (x[far, 0] - x[:, 0].min())
    ti = _integrator(scheme, _assembler(engine, kind, "neo_hookean"), kind, 1e-4, newton_tol=1e-10, max_it=5)
    ti.set_state(u0)
    with pytest.raises(fa.DynamicsError) as ei:
        ti.step(3)
    assert ei.value.code == FH_DYNAMICS_NONFINITE and ei.value.steps_done == 0


def _hard_step():
    """Tet4 NeoHookean under Newmark at 40 dt: a load so small that one Newton iteration meets the tolerance for two steps, then 1000 times
    that load at once, which one iteration does not solve (sized on the CPU reference)"""
    kind = "TET4"
    dt = 40.0 * _modal(kind, "elastic")["dt"]
    f, lf = _body_load(kind, 2.0e4), np.array([0.0, 1e-3, 1e-3, 1.0])
    return kind, dt, f, lf, 1e-6 * np.linalg.norm(f) * 0.25 * dt * dt


@pytest.mark.gpu
def test_newton_failure_leaves_the_last_completed_step(engine, oracle):
    """newton_max_iterations = 1 under a load that needs more: the call ends with FH_NEWTON_MAX_ITERATIONS at the first hard step and the
    state is that of the steps completed before it (the reference's, stopped the same way)"""
    kind, dt, f, lf, tol_n = _hard_step()
    prob = _problem(oracle, kind, "neo_hookean", f, lf)
    z = np.zeros_like(f)
    v0 = np.zeros_like(f)
    st, ur, vr, ar, _, done, _ = dr.implicit(prob, "newmark", z, v0, dt, 5, 0, tol=tol_n, max_it=1)
    assert st == "maxit" and done == 2 and np.abs(ur).max() > 0
    ti = _integrator("newmark", _assembler(engine, kind, "neo_hookean"), kind, dt, f, lf, newton_tol=tol_n, max_it=1)
    ti.set_state(z, v0)
    with pytest.raises(fa.MaximumIterationsReached) as ei:
        ti.step(5)
    assert ei.value.code == _ffi.FH_NEWTON_MAX_ITERATIONS and ei.value.steps_done == 2
    u, v, a, time, step = ti.state()
    assert step == 2 and abs(time - 2 * dt) <= 1e-14 * time
    assert np.abs(u - ur).max() <= 1e-8 * np.abs(ur).max() and np.abs(v - vr).max() <= 1e-8 * np.abs(vr).max()


# ------------------------------------------------------------------------------------------ 6. stable_dt
# d_perm of the reference's omega_max^2 after 30 iterations (rounding level: the floor of 1e-13 holds), 0, the tolerance
STABLE_DT_TOLERANCE = {
    ("HEX8", "elastic"): (0.0e+00, 0.0, 1.0e-13),
    ("TET4", "elastic"): (2.1e-16, 0.0, 1.0e-13),
    ("QUAD4", "laplace"): (1.4e-16, 0.0, 1.0e-13),
    ("QUAD9", "laplace"): (3.7e-16, 0.0, 1.0e-13),
    ("HEX27", "elastic"): (1.4e-16, 0.0, 1.0e-13),
}


@pytest.mark.gpu
@pytest.mark.parametrize("kind,op", [("HEX8", "elastic"), ("TET4", "elastic"), ("QUAD4", "laplace"), ("QUAD9", "laplace"), ("HEX27", "elastic")])
def test_stable_dt(engine, oracle, kind, op):
    """omega_max^2 after 30 iterations is the reference's power iteration from the same start vector (tolerance: the reference against its
    permuted self, margin 20); it never exceeds the dense lambda_max by more than 1e-10 relative; a central-difference run at
    0.9 dt_crit of the dense pencil keeps the invariant of the linear scheme -- which decides the support of Quad9 and Hex27"""
    md = _modal(kind, op)
    prob = _problem(oracle, kind, op)
    z = np.zeros(prob.n)
    want = dr.power_iteration(prob, z, 30)
    d_perm = abs(dr.power_iteration(_problem(oracle, kind, op, perm=7), z, 30) - want) / want
    tol = _check_constants((kind, op), d_perm, 0.0, max(20.0 * d_perm, 1e-13), STABLE_DT_TOLERANCE)
    ti = _integrator("central", _assembler(engine, kind, op), kind, 0.9 * 2.0 / np.sqrt(md["lam_max"]))
    ti.set_state(z)
    om, dtc = ti.stable_dt(30)
    print(f"{kind} {op}: omega_max^2 {om * om:.6e}, reference {want:.6e}, dense {md['lam_max']:.6e}")
    assert abs(om * om - want) <= tol * want
    assert om * om <= md["lam_max"] * (1.0 + 1e-10) and dtc == 2.0 / om
    omv, V = md["central"]
    u0, v0 = V[:, 0], 0.5 * omv[1] * V[:, 1]
    dt = 0.9 * 2.0 / np.sqrt(md["lam_max"])
    ti.set_state(u0, v0)
    m = prob.lumped()
    assert (m[prob.free] > 0).all()
    a0 = ti.state()[2]
    H = [0.5 * float(np.sum(m * v0 * v0)) + prob.energy(u0) - dt * dt / 8.0 * float(np.sum(m * a0 * a0))]
    for _ in range(8):
        rec = ti.step(8)
        a = ti.state()[2]
        H.append(rec.kinetic[-1] + rec.stored[-1] - dt * dt / 8.0 * float(np.sum(m * a * a)))
    drift = np.abs(np.array(H) - H[0]).max() / abs(H[0])
    print(f"{kind} {op}: relative drift of the invariant at 0.9 dt_crit {drift:.3e}")
    assert drift <= 1e-11


# ------------------------------------------------------------------------------------------ 7. reproducibility and restart
def _run_cut(engine, scheme, cut, device=False):
    kind = "HEX8"
    dt = _modal(kind, "elastic")["dt"]
    f, lf = _body_load(kind, LOAD[kind]), _ramp()
    ti = _integrator(scheme, _assembler(engine, kind, "neo_hookean"), kind, dt, f, lf, newton_tol=_newton_tol(f, dt, scheme))
    if device:
        import torch

        ti.with_load(torch.from_numpy(f).to("cuda:0"), lf)
        ti.set_state(torch.zeros(len(f), dtype=torch.float64, device="cuda:0"))
    else:
        ti.set_state(np.zeros_like(f))
    steps = 24 if scheme == "central" else 6
    if cut == "one":
        rec = ti.step(steps)
    elif cut == "three":
        for _ in range(3):
            rec = ti.step(steps // 3)
    else:
        rec = ti.step(steps, record_every=5)
    u, v, a, time, step = ti.state(device=device)
    if device:
        u, v, a = (t.cpu().numpy() for t in (u, v, a))
    assert step == steps
    return u, v, a, _records(rec)[-1], time


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["central", "newmark"])
def test_runs_repeat_and_restart_bit_for_bit(engine, scheme):
    """two identical runs, and one run cut three ways (one call; three calls; one call with a record every 5 steps), give identical bits in
    u, v, a and the final record: a fused kick and drift that disagreed with the stand-alone one would show here.  The host and the _dev
    entry points return the same bits."""
    base = _run_cut(engine, scheme, "one")
    assert np.isfinite(base[0]).all() and np.abs(base[0]).max() > 0
    for cut, device in (("one", False), ("three", False), ("records", False), ("one", True)):
        other = _run_cut(engine, scheme, cut, device)
        for name, p, q in zip(("u", "v", "a", "record", "time"), base, other):
            assert np.array_equal(np.asarray(p), np.asarray(q)), (scheme, cut, device, name)
