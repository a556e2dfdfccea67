"""Rayleigh damping of the second-order time integrators (fh_dynamics_set_damping, TimeIntegrator.with_damping): central differences,
Newmark and backward Euler with C = eta_m M + eta_k T(u) against the NumPy statement of tests/damping_reference.py, which integrates the
unfolded equations and is pinned here on the CPU against the closed forms of a single eigenmode."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import fenris_amd as fa
from fenris_amd import _ffi, quadrature

import damping_reference as dmp
import dynamics_reference as dr

LAME = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.3))
RHO = 1000.0
FH_BAD_ARGUMENT, FH_UNSUPPORTED = 2, 6
OKIND = {"QUAD4": 0, "HEX8": 1, "TET4": 2, "HEX27": 3, "TRI3": 4}
SCHEMES = ("central", "newmark", "euler")
FUSED = ("HEX8", "TET4", "QUAD4", "TRI3")
NEW = ("fh_dynamics_set_damping", "fh_dynamics_damping")
# which part of C a case carries
PARTS = {"mass": (1.0, 0.0), "stiffness": (0.0, 1.0), "both": (1.0, 1.0)}


@pytest.fixture()
def engine():
    eng = fa.Engine(0)
    yield eng
    eng.close()


# ------------------------------------------------------------------------------------------ meshes, problems, integrators
@functools.lru_cache(maxsize=None)
def _mesh(kind):
    """Hex8 3^3, the Tet4 grid at resolution 2, Quad4 and Tri3 4^2; Hex8 7^3 (343 elements: two tiles, so node sums cross a tile boundary);
    Hex27 and a Hex8 2^3 box for the routes off the tiles"""
    P, T, Q = fa.procedural, quadrature.tensor, quadrature.total_order
    make = {"HEX8": (lambda: P.create_unit_box_uniform_hex_mesh_3d(3), T.hexahedron_gauss(2)),
            "TET4": (lambda: P.create_unit_box_uniform_tet_mesh_3d(2), Q.tetrahedron(2)),
            "QUAD4": (lambda: P.create_unit_square_uniform_quad_mesh_2d(4), T.quadrilateral_gauss(2)),
            "TRI3": (lambda: P.create_unit_square_uniform_tri_mesh_2d(4), Q.triangle(2)),
            "HEX8_7": (lambda: P.create_unit_box_uniform_hex_mesh_3d(7), T.hexahedron_gauss(2)),
            "HEX8_2": (lambda: P.create_unit_box_uniform_hex_mesh_3d(2), T.hexahedron_gauss(2)),
            "HEX27": (lambda: fa.hex27_mesh_from_hex8(P.create_unit_box_uniform_hex_mesh_3d(2)), T.hexahedron_gauss(3))}
    gen, (w, p) = make[kind]
    return gen(), np.asarray(w), np.asarray(p)


def _okind(kind):
    return OKIND[kind.split("_")[0]]


def _clamp(m):
    x = m.vertices[:, 0]
    return np.where(np.isclose(x, x.min()))[0]


def _lame(op, d):
    return LAME.for_stable_neo_hookean(d) if op == "stable_neo_hookean" else LAME


class _StableProblem(dr.Problem):
    """dynamics_reference's problem on the long-double reference of the Stable Neo-Hookean law (tests/stable_neo_hookean_reference.py),
    rounded to double; perm: another order of the elements"""

    def __init__(self, kind, m, w, p, f=None, load_factor=None, perm=None):
        import stable_neo_hookean_reference as snh

        self.snh = snh
        conn = np.asarray(m.connectivity)
        self.conn = conn if perm is None else conn[np.random.default_rng(perm).permutation(len(conn))]
        self.kind, self.vertices, self.w, self.p, self.rho = kind.split("_")[0], np.asarray(m.vertices), w, p, RHO
        self.d = self.s = self.vertices.shape[1]
        self.lame = _lame("stable_neo_hookean", self.d)
        self.N = len(self.vertices)
        self.n = self.s * self.N
        self.free = np.ones(self.n, dtype=bool)
        for k in range(self.s):
            self.free[self.s * _clamp(m) + k] = False
        self.f = np.zeros(self.n) if f is None else np.asarray(f, dtype=np.float64).reshape(-1)
        self.load_factor = None if load_factor is None else np.asarray(load_factor, dtype=np.float64)
        self.direct, self._mass = "sparse", None

    def ref(self, u):
        return self.snh.Reference(self.kind, self.vertices, self.conn, self.w, self.p, u, self.lame.mu, self.lame.lambda_, rho=self.rho)

    def residual(self, u):
        return self.ref(u).residual().astype(np.float64)

    def energy(self, u):
        return float(self.ref(u).energy())

    def _csr(self, ref, which):
        import scipy.sparse as sp

        ro, ci = ref.pattern()
        return sp.csr_matrix((ref.csr_values(ro, ci, which).astype(np.float64), ci, ro), shape=(self.n, self.n))

    def tangent(self, u):
        return self._csr(self.ref(u), "K")

    def mass(self):
        if self._mass is None:
            self._mass = self._csr(self.ref(np.zeros(self.n)), "M")
        return self._mass


def _problem(oracle, kind, op, f=None, load_factor=None, groups=None, direct="sparse", perm=None, obstacles=()):
    """the reference's problem; perm: a permutation of the connectivity rows (another summation order in r, nothing else)"""
    m, w, p = _mesh(kind)
    if op == "stable_neo_hookean":
        return _StableProblem(kind, m, w, p, f, load_factor, perm)
    if groups is None:
        groups = [(np.asarray(m.connectivity), w, p)]
    if perm is not None:
        groups = [(c[np.random.default_rng(perm + g).permutation(len(c))], wg, pg) for g, (c, wg, pg) in enumerate(groups)]
    oop = {"laplace": oracle.LAPLACE, "elastic": oracle.LINEAR_ELASTIC, "neo_hookean": oracle.NEO_HOOKEAN, "stvk": oracle.STVK}[op]
    args = (oracle, _okind(kind), oop, m.vertices, groups)
    kw = dict(params=None if op == "laplace" else LAME.as_pair(), rho=RHO, dirichlet=_clamp(m), f=f, load_factor=load_factor, direct=direct)
    if obstacles:
        import contact_reference as cr

        return cr.ContactProblem(*args, obstacles=obstacles, **kw)
    return dr.Problem(*args, **kw)


def _operator(op):
    return {"laplace": fa.LaplaceOperator(), "elastic": fa.MaterialEllipticOperator(fa.LinearElasticMaterial()),
            "neo_hookean": fa.MaterialEllipticOperator(fa.NeoHookeanMaterial()), "stvk": fa.MaterialEllipticOperator(fa.StVKMaterial()),
            "stable_neo_hookean": fa.MaterialEllipticOperator(fa.StableNeoHookeanMaterial())}[op]


def _assembler(engine, kind, op, qt=None):
    m, w, p = _mesh(kind)
    d = m.vertices.shape[1]
    s = 1 if op == "laplace" else d
    if qt is None:
        qt = fa.UniformQuadratureTable.from_points_and_weights(p, w)
        qt = qt if op == "laplace" else qt.with_uniform_data(_lame(op, d))
    return (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(m).with_operator(_operator(op)).with_quadrature_table(qt)
            .with_u(np.zeros(s * m.num_nodes())).build())


def _integrator(scheme, asm, kind, dt, damping, f=None, load_factor=None, newton_tol=1e-8, max_it=None, linear_rel_tol=1e-12):
    clamp = _clamp(_mesh(kind)[0])
    if scheme == "central":
        ti = fa.CentralDifference(asm, RHO, dt)
    else:
        ti = fa.Newmark(asm, RHO, dt) if scheme == "newmark" else fa.BackwardEuler(asm, RHO, dt)
        ti.with_newton(fa.NewtonSettings(max_it, newton_tol), linear_rel_tol=linear_rel_tol)
    ti.with_dirichlet_nodes(clamp).with_load(f, load_factor)
    return ti if damping is None else ti.with_damping(*damping)


@functools.lru_cache(maxsize=None)
def _modal(kind, op):
    """dense pencils of the clamped body at u = 0: dt = 0.5 * 2 / omega_max of (K, diag m); the lowest two modes and the highest of
    (K, diag m) and of (K, M); K and M on the free dofs"""
    from oracle import oracle as o

    o.lib()
    prob = _problem(o, kind, op, direct="dense")
    z = np.zeros(prob.n)
    wc, Vc = dr.dense_pencil(prob, z, False)
    wl, Vl = dr.dense_pencil(prob, z, True)
    fr = prob.free
    return {"dt": 0.5 * 2.0 / np.sqrt(wl[-1]), "om_max": np.sqrt(wl[-1]), "central": (np.sqrt(wl[:2]), Vl[:, :2]), "newmark": (np.sqrt(wc[:2]), Vc[:, :2]),
            "euler": (np.sqrt(wc[:2]), Vc[:, :2]), "top": (np.sqrt(wl[-1]), Vl[:, -1]), "K": prob.tangent(z)[fr][:, fr].toarray(),
            "M": prob.mass()[fr][:, fr].toarray(), "Kphi": np.linalg.norm(prob.tangent(z) @ Vc[:, 0])}


def _mode_damping(md, scheme, part):
    """coefficients that damp the lowest mode visibly and keep central differences at dt = 1 / omega_max stable: eta_m = 0.2 omega_0,
    eta_k = 0.5 / omega_max (the limit (omega dt)^2 + 2 eta_k omega^2 dt <= 4 reads 1 + 1 <= 4 for the highest mode)"""
    sm, sk = PARTS[part]
    return sm * 0.2 * md[scheme][0][0], sk * 0.5 / md["om_max"]


def _kappa(md, scheme, dt, eta_m, eta_k):
    """the condition number of the matrix of the implicit step, alpha M + beta' K"""
    g, b = (1.0, dt * dt) if scheme == "euler" else (0.5, 0.25 * dt * dt)
    return np.linalg.cond((1.0 + eta_m * g * dt) * md["M"] + (b + eta_k * g * dt) * md["K"])


def _reference_run(prob, scheme, u0, v0, dt, steps, record_every, damping, tol=1e-8):
    if scheme == "central":
        return dmp.central_difference(prob, u0, v0, dt, steps, damping[0], damping[1], record_every)
    st, u, v, a, rec, done, _ = dmp.implicit(prob, scheme, u0, v0, dt, steps, damping[0], damping[1], record_every, tol=tol)
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


def _assert_parity(got, ref, tol, what=""):
    worst = 0.0
    for name, p, q in zip("uva", got[:3], ref[:3]):
        err = np.abs(p - q).max() / max(np.abs(q).max(), 1e-300)
        print(f"{what} {name}: {err:.3e} (tol {tol:.3e})")
        worst = max(worst, err)
    for c, name in enumerate(("kinetic", "stored", "load_potential", "time")):
        err = np.abs(got[3][:, c] - ref[3][:, c]).max() / max(np.abs(ref[3][:, c]).max(), 1e-300)
        print(f"{what} {name}: {err:.3e} (tol {tol:.3e})")
        worst = max(worst, err)
    assert worst <= tol, (what, worst, tol)


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


def _ramp():
    return np.linspace(0.0, 1.0, 8)


# ------------------------------------------------------------------------------------------ 8. declarations (no GPU)
def test_damping_entry_points_are_declared():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "fenris_hip.h")).read()
    rs = open(os.path.join(root, "bindings", "fenris_hip_sys.rs")).read()
    for name in NEW:
        assert name in _ffi.exported_symbols() and name + "(" in hdr and "fn " + name + "(" in rs
    assert "int fh_dynamics_set_damping(fh_dynamics*, double eta_mass, double eta_stiffness);" in hdr
    assert "int fh_dynamics_damping(fh_dynamics*, double* eta_mass, double* eta_stiffness);" in hdr
    for cls in (fa.CentralDifference, fa.Newmark, fa.BackwardEuler):
        assert callable(cls.with_damping)
    assert fa.RayleighDamping(0.5, 1e-4) == fa.RayleighDamping(mass=0.5, stiffness=1e-4) and fa.RayleighDamping() == fa.RayleighDamping(0.0, 0.0)


# ------------------------------------------------------------------------------------------ 1. the reference is right (no GPU)
@pytest.mark.parametrize("part", list(PARTS))
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("kind,op", [("HEX8_2", "elastic"), ("TET4", "elastic"), ("QUAD4", "laplace")])
def test_reference_meets_the_damped_closed_forms(oracle, kind, op, scheme, part):
    """u_0 = phi, v_0 = 0, f = 0 on one eigenmode of the scheme's dense pencil: the vector reference follows the scalar closed form (the
    powers of the 2 x 2 step matrix; the damped Newmark and backward Euler recurrences) to 1e-10 max|phi| over 32 steps"""
    md = _modal(kind, op)
    om, V = md[scheme]
    phi, dt = V[:, 0], md["dt"]
    damping = _mode_damping(md, scheme, part)
    prob = _problem(oracle, kind, op, direct="dense")
    decay = dmp.closed_form(scheme, om[0], dt, 32, *damping) / dr.closed_form(scheme, om[0], dt, 32)
    print(f"{kind} {op} {scheme} {part}: damped / undamped factor after 32 steps {decay:.6f}")
    assert abs(decay - 1.0) > 1e-6   # the damping shows at the bar of this test
    for n in (1, 2, 7, 32):
        u = _reference_run(prob, scheme, phi, np.zeros_like(phi), dt, n, 0, damping, tol=1e-12 * md["Kphi"])[0]
        assert np.abs(u - dmp.closed_form(scheme, om[0], dt, n, *damping) * phi).max() <= 1e-10 * np.abs(phi).max()


def test_from_ratios_reproduces_both_ratios():
    for xi1, w1, xi2, w2 in ((0.02, 10.0, 0.05, 300.0), (0.05, 3.0, 0.05, 40.0), (0.01, 123.4, 0.2, 9876.5)):
        rd = fa.RayleighDamping.from_ratios(xi1, w1, xi2, w2)
        assert rd.mass >= 0.0 and rd.stiffness >= 0.0
        for xi, w in ((xi1, w1), (xi2, w2)):
            assert abs(rd.mass / (2.0 * w) + rd.stiffness * w / 2.0 - xi) <= 1e-15 and abs(rd.ratio(w) - xi) <= 1e-15
    with pytest.raises(ValueError):
        fa.RayleighDamping.from_ratios(0.01, 10.0, 0.5, 11.0)   # needs eta_m < 0
    with pytest.raises(ValueError):
        fa.RayleighDamping.from_ratios(0.01, 10.0, 0.01, 10.0)


# ------------------------------------------------------------------------------------------ 2. the stability limit (no GPU)
@pytest.mark.parametrize("xi", [0.1, 1.0])
def test_stability_limit_of_the_highest_mode(oracle, xi):
    """eta_k with xi = eta_k omega_max / 2: the reference's recurrence on the highest mode of (K, diag m) stays bounded at 0.999 dt_crit
    over 2000 steps and grows at 1.001 dt_crit, dt_crit = (2 / omega_max)(sqrt(1 + xi^2) - xi); eta_m does not move the limit"""
    kind, op = "QUAD4", "laplace"
    md = _modal(kind, op)
    om, phi = md["top"]
    eta_k = 2.0 * xi / om
    dtc = dmp.dt_crit(om, eta_k)
    assert abs((om * dtc) ** 2 + 2.0 * eta_k * om * om * dtc - 4.0) <= 1e-12
    prob = _problem(oracle, kind, op, direct="dense")
    for eta_m in (0.0, 0.05 * om):
        for s in (0.999, 1.001):
            # (u_0 = phi splits over the two roots of the mode: the amplitudes after 1000 and after 2000 steps show which way the larger goes)
            amp = [np.abs(dmp.central_difference(prob, phi, np.zeros_like(phi), s * dtc, n, eta_m, eta_k)[0]).max() / np.abs(phi).max()
                   for n in (1000, 2000)]
            rho = np.abs(np.linalg.eigvals(dmp.explicit_step_matrix(om, s * dtc, eta_m, eta_k))).max()   # the scalar recurrence says the same
            print(f"xi {xi} eta_m {eta_m:.3e} at {s} dt_crit: |u_1000|, |u_2000| over |u_0| = {amp[0]:.3e}, {amp[1]:.3e}; spectral radius {rho:.8f}")
            assert (rho <= 1.0 + 1e-12) == (s < 1.0)
            if s < 1.0:
                assert amp[0] <= 1.0 + 1e-9 and amp[1] <= 1.0 + 1e-9
            else:
                assert amp[1] >= 5.0 * amp[0] and amp[1] >= rho ** 1000 / 2.0 * amp[0]


# ------------------------------------------------------------------------------------------ 3. single-mode closed forms on the device
@pytest.mark.gpu
@pytest.mark.parametrize("part", list(PARTS))
@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("op", ["laplace", "elastic"])
@pytest.mark.parametrize("kind", FUSED)
def test_single_mode_closed_forms(engine, kind, op, scheme, part):
    """32 steps on one eigenmode with the tolerances of test_dynamics.test_single_mode_closed_forms: central differences 1e-10 max|phi|; the
    implicit schemes 10 steps kappa linear_rel_tol max|phi|, kappa of alpha M + beta' K"""
    md = _modal(kind, op)
    om, V = md[scheme]
    phi, dt, steps = V[:, 0], md["dt"], 32
    damping = _mode_damping(md, scheme, part)
    tol = 1e-10 if scheme == "central" else 10.0 * steps * _kappa(md, scheme, dt, *damping) * 1e-12
    ti = _integrator(scheme, _assembler(engine, kind, op), kind, dt, damping, newton_tol=1e-12 * md["Kphi"])
    ti.set_state(phi)
    worst = 0.0
    for n in range(1, steps + 1):
        rec = ti.step(1)
        assert rec.steps_done == 1 and len(rec.time) == 1
        u = ti.state()[0]
        worst = max(worst, np.abs(u - dmp.closed_form(scheme, om[0], dt, n, *damping) * phi).max() / np.abs(phi).max())
    print(f"{kind} {op} {scheme} {part}: worst error {worst:.3e} of max|phi| (tol {tol:.3e})")
    assert worst <= tol
    got = ti.damping()
    assert (got.mass, got.stiffness) == damping


# ------------------------------------------------------------------------------------------ 4. trajectory parity with the reference
# The load: a ramp over the first 8 steps, then held, spread over all nodes along +x and sized on the CPU reference so that the peak
# displacement of the 16 steps is some per cent of the body's length.  The coefficients: eta_m dt = 0.1 and eta_k = 0.2 dt at
# dt = 1 / omega_max of the linear-elastic body (eta_k omega_max = 0.2: far inside the explicit limit), scaled by the case's part of C.
LOAD = {"HEX8": 1.3e5, "TET4": 1.3e5, "QUAD4": 4.0e5, "TRI3": 4.0e5, "HEX8_7": 1.3e5, "HEX27": 1.1e5, "HEX8_2": 1.3e5}
NONLINEAR = ("neo_hookean", "stvk", "stable_neo_hookean")
EXPLICIT_CASES = [(k, o, "central", "both") for k in FUSED for o in ("elastic",) + NONLINEAR]
IMPLICIT_CASES = ([(k, o, s, "both") for k, o in (("HEX8", "elastic"), ("TET4", "elastic"), ("QUAD4", "laplace"), ("TRI3", "elastic")) for s in ("newmark", "euler")]
                  + [(k, o, s, "mass") for k, o in (("HEX8", "neo_hookean"), ("TET4", "stvk"), ("QUAD4", "stable_neo_hookean")) for s in ("newmark", "euler")])
# Measured on the CPU with the reference alone (_measured_tolerance): d_perm, d_newton and the resulting tolerance 20 (d_perm + d_newton),
# floored at 1e-13, per case.  The tests measure them again and assert that they stay within a factor 10 of these.
TRAJECTORY_TOLERANCE = {
    ('HEX8', 'elastic', 'central', 'both'): (1.6e-14, 0.0e+00, 3.2e-13),
    ('HEX8', 'neo_hookean', 'central', 'both'): (1.1e-14, 0.0e+00, 2.3e-13),
    ('HEX8', 'stvk', 'central', 'both'): (2.7e-14, 0.0e+00, 5.4e-13),
    ('HEX8', 'stable_neo_hookean', 'central', 'both'): (0.0e+00, 0.0e+00, 1.0e-13),
    ('TET4', 'elastic', 'central', 'both'): (2.0e-14, 0.0e+00, 3.9e-13),
    ('TET4', 'neo_hookean', 'central', 'both'): (1.6e-14, 0.0e+00, 3.3e-13),
    ('TET4', 'stvk', 'central', 'both'): (2.5e-14, 0.0e+00, 5.0e-13),
    ('TET4', 'stable_neo_hookean', 'central', 'both'): (2.3e-17, 0.0e+00, 1.0e-13),
    ('QUAD4', 'elastic', 'central', 'both'): (9.1e-15, 0.0e+00, 1.8e-13),
    ('QUAD4', 'neo_hookean', 'central', 'both'): (1.2e-14, 0.0e+00, 2.4e-13),
    ('QUAD4', 'stvk', 'central', 'both'): (1.9e-14, 0.0e+00, 3.7e-13),
    ('QUAD4', 'stable_neo_hookean', 'central', 'both'): (1.9e-18, 0.0e+00, 1.0e-13),
    ('TRI3', 'elastic', 'central', 'both'): (9.5e-15, 0.0e+00, 1.9e-13),
    ('TRI3', 'neo_hookean', 'central', 'both'): (3.1e-14, 0.0e+00, 6.2e-13),
    ('TRI3', 'stvk', 'central', 'both'): (3.6e-14, 0.0e+00, 7.2e-13),
    ('TRI3', 'stable_neo_hookean', 'central', 'both'): (0.0e+00, 0.0e+00, 1.0e-13),
    ('HEX8', 'elastic', 'newmark', 'both'): (6.2e-14, 0.0e+00, 1.2e-12),
    ('HEX8', 'elastic', 'euler', 'both'): (4.7e-14, 0.0e+00, 9.4e-13),
    ('TET4', 'elastic', 'newmark', 'both'): (3.3e-14, 0.0e+00, 6.5e-13),
    ('TET4', 'elastic', 'euler', 'both'): (2.5e-14, 0.0e+00, 5.1e-13),
    ('QUAD4', 'laplace', 'newmark', 'both'): (1.6e-16, 0.0e+00, 1.0e-13),
    ('QUAD4', 'laplace', 'euler', 'both'): (4.7e-15, 0.0e+00, 1.0e-13),
    ('TRI3', 'elastic', 'newmark', 'both'): (1.1e-13, 0.0e+00, 2.2e-12),
    ('TRI3', 'elastic', 'euler', 'both'): (3.9e-14, 0.0e+00, 7.7e-13),
    ('HEX8', 'neo_hookean', 'newmark', 'mass'): (1.1e-13, 1.2e-11, 2.4e-10),
    ('HEX8', 'neo_hookean', 'euler', 'mass'): (2.4e-14, 2.4e-11, 4.7e-10),
    ('TET4', 'stvk', 'newmark', 'mass'): (6.2e-14, 7.2e-12, 1.4e-10),
    ('TET4', 'stvk', 'euler', 'mass'): (2.1e-14, 4.5e-12, 9.1e-11),
    ('QUAD4', 'stable_neo_hookean', 'newmark', 'mass'): (3.1e-17, 4.7e-11, 9.3e-10),
    ('QUAD4', 'stable_neo_hookean', 'euler', 'mass'): (3.0e-18, 4.8e-11, 9.6e-10),
}


def _dt(kind):
    return _modal(kind, "elastic")["dt"]


def _damping_for(dt, part):
    sm, sk = PARTS[part]
    return sm * 0.1 / dt, sk * 0.2 * dt


def _newton_tol(f, dt, scheme):
    """1e-11 ||beta dt^2 f||: both the reference and the device then stop at rounding level"""
    return 1e-11 * np.linalg.norm(f) * {"central": 0.0, "newmark": 0.25, "euler": 1.0}[scheme] * dt * dt


def _measured_tolerance(oracle, kind, op, scheme, f, lf, dt, damping, tol, u0=None, v0=None, **kw):
    """the reference against itself, as tests/test_dynamics.py takes it: d_perm from a permuted connectivity, d_newton from a Newton
    tolerance 100 times smaller; the tolerance is 20 (d_perm + d_newton), never below 1e-13"""
    n = _problem(oracle, kind, op).n
    u0 = np.zeros(n) if u0 is None else u0
    v0 = np.zeros(n) if v0 is None else v0
    ref = _reference_run(_problem(oracle, kind, op, f, lf, **kw), scheme, u0, v0, dt, 16, 4, damping, tol)
    perm = _reference_run(_problem(oracle, kind, op, f, lf, perm=7, **kw), scheme, u0, v0, dt, 16, 4, damping, tol)
    d_perm = _rel_diff(ref, perm)
    d_newton = 0.0
    if scheme != "central":
        d_newton = _rel_diff(ref, _reference_run(_problem(oracle, kind, op, f, lf, **kw), scheme, u0, v0, dt, 16, 4, damping, tol / 100.0))
    return ref, d_perm, d_newton, max(20.0 * (d_perm + d_newton), 1e-13)


def _check_constants(key, d_perm, d_newton, tol, table=None):
    c_perm, c_newton, c_tol = (TRAJECTORY_TOLERANCE if table is None else table)[key]
    print(f"{key}: d_perm {d_perm:.3e} (constant {c_perm:.3e}), d_newton {d_newton:.3e} ({c_newton:.3e}), tolerance {tol:.3e} ({c_tol:.3e})")
    assert c_tol / 10.0 <= tol <= 10.0 * c_tol, (key, d_perm, d_newton, tol)
    return c_tol


def _device_run(ti, n, u0=None, v0=None):
    ti.set_state(np.zeros(n) if u0 is None else u0, v0)
    rec = ti.step(16, record_every=4)
    assert rec.steps_done == 16 and len(rec.time) == 4 and rec.stats[0] == 16 and rec.stats[4] == 4
    u, v, a, _, step = ti.state()
    assert step == 16
    return u, v, a, _records(rec)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,op,scheme,part", EXPLICIT_CASES + IMPLICIT_CASES)
def test_trajectory_parity_with_the_reference(engine, oracle, kind, op, scheme, part):
    """16 steps under the ramped load with a record every 4: u, v, a and every record row against the reference.  With a linear operator
    the reference's one direct solve per step leaves rounding only and d_newton is 0, so the device's inner PCG is asked for rounding
    level too (linear_rel_tol = 1e-14; at 1e-12, sixteen inexact solves show in a = (u - u_ref) / (beta dt^2) at 1.5e-12); with a nonlinear
    operator d_newton covers the inexact solves and the PCG stays at 1e-12 as in tests/test_dynamics.py"""
    dt = _dt(kind)
    damping = _damping_for(dt, part)
    f, lf = _body_load(kind, LOAD[kind]), _ramp()
    if op == "laplace":
        f = f[0::_mesh(kind)[0].vertices.shape[1]].copy()
    tol_n = _newton_tol(f, dt, scheme)
    ref, d_perm, d_newton, tol = _measured_tolerance(oracle, kind, op, scheme, f, lf, dt, damping, tol_n)
    tol = _check_constants((kind, op, scheme, part), d_perm, d_newton, tol)
    ti = _integrator(scheme, _assembler(engine, kind, op), kind, dt, damping, f, lf, newton_tol=tol_n,
                     linear_rel_tol=1e-14 if op in ("laplace", "elastic") else 1e-12)
    got = _device_run(ti, len(f))
    if scheme == "central":
        assert engine.last_kernel_name() != "" and ti.damping().stiffness > 0.0
    _assert_parity(got, ref, tol, f"{kind} {op} {scheme} {part}")
    x = _mesh(kind)[0].vertices[:, 0]
    peak = np.abs(got[0]).max() / (x.max() - x.min())
    print(f"{kind} {op} {scheme} {part}: peak displacement {peak:.3f} of the body's length")
    assert op == "laplace" or 0.01 <= peak <= 0.3


def _rules_case(engine):
    m, w, p = _mesh("HEX8_2")
    conn = np.asarray(m.connectivity)
    w2, p2 = (np.asarray(a) for a in quadrature.tensor.hexahedron_gauss(3))
    emap = (np.arange(len(conn)) % 2).astype(np.uint64)
    qt = fa.compact_quadrature_table([p, p2], [w, w2], [[LAME] * len(w), [LAME] * len(w2)], emap)
    return _assembler(engine, "HEX8_2", "neo_hookean", qt=qt), [(conn[emap == 0], w, p), (conn[emap == 1], w2, p2)]


FLOOR = [("half_space", (0.0, 0.0, -0.02), (0.0, 0.0, 1.0), 2.0e3)]
OTHER_TOLERANCE = {
    'hex27_central': (5.5e-14, 0.0e+00, 1.1e-12),
    'rules_central': (3.3e-15, 0.0e+00, 1.0e-13),
    'obstacle_central': (6.5e-15, 0.0e+00, 1.3e-13),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["hex27_central", "rules_central", "obstacle_central"])
def test_other_routes_parity(engine, oracle, case):
    """central differences with both coefficients off the fused route -- Hex27, a Hex8 rule-set table (the residual and eta_k T(u) v_h are
    summed, then k_dynamics_update) -- and on it with an obstacle set, whose term stays out of C: a block that starts 0.01 inside a floor,
    moving into it"""
    kind = {"hex27_central": "HEX27", "rules_central": "HEX8_2", "obstacle_central": "HEX8_2"}[case]
    dt = _dt(kind)
    damping = _damping_for(dt, "both")
    f, lf = _body_load(kind, LOAD[kind]), _ramp()
    kw, u0, v0 = {}, None, None
    if case == "rules_central":
        asm, kw["groups"] = _rules_case(engine)
    else:
        asm = _assembler(engine, kind, "neo_hookean")
    if case == "obstacle_central":
        import contact_reference as cr

        kw["obstacles"] = FLOOR
        dt = 0.5 * dt   # (the floor's penalty stiffens the bottom nodes)
        damping = _damping_for(dt, "both")
        u0, v0 = np.zeros(len(f)), np.zeros(len(f))
        u0[2::3], v0[2::3] = -0.03, -1.0
    ref, d_perm, d_newton, tol = _measured_tolerance(oracle, kind, "neo_hookean", "central", f, lf, dt, damping, 0.0, u0=u0, v0=v0, **kw)
    tol = _check_constants(case, d_perm, d_newton, tol, OTHER_TOLERANCE)
    ti = _integrator("central", asm, kind, dt, damping, f, lf)
    if case == "obstacle_central":
        ti.with_obstacles(fa.Obstacles([fa.HalfSpace(*FLOOR[0][1:])]))
    got = _device_run(ti, len(f), u0, v0)
    _assert_parity(got, ref, tol, case)
    if case == "obstacle_central":
        gap = cr.gap(FLOOR, _mesh(kind)[0].vertices, got[0]).min()
        print(f"deepest gap {gap:.4f}")
        assert gap < 0.0   # the block is in the floor
    ti.close()
    # the name of the step's launch: a_0 of a second integrator
    t2 = _integrator("central", asm, kind, dt, damping, f, lf)
    if case == "obstacle_central":
        t2.with_obstacles(fa.Obstacles([fa.HalfSpace(*FLOOR[0][1:])]))
    t2.set_state(np.zeros(len(f)) if u0 is None else u0, v0)
    t2.state()
    want = {"hex27_central": "k_residual_elements + k_vector_from_elements_soa + k_dynamics_update",
            "rules_central": "k_residual_elements + k_vector_from_elements_soa + k_dynamics_update",
            "obstacle_central": "k_damped_pass_tiled + k_dynamics_from_partials"}[case]
    assert engine.last_kernel_name() == want, engine.last_kernel_name()
    t2.close()


# ------------------------------------------------------------------------------------------ 5. invariants
@pytest.mark.gpu
@pytest.mark.parametrize("part", list(PARTS))
@pytest.mark.parametrize("kind,op", [("HEX8", "elastic"), ("TET4", "elastic"), ("QUAD4", "laplace"), ("TRI3", "laplace")])
def test_newmark_energy_balance(engine, oracle, kind, op, part):
    """Newmark (1/4, 1/2), linear operator, no load, 64 steps from u_0 = phi_0, v_0 = omega_1 phi_1 / 2: kinetic + stored never increases,
    and E_{n+1} - E_n = -dt vbar . C vbar with vbar = (v_n + v_{n+1}) / 2, both within the rounding bound 10 steps kappa linear_rel_tol of
    test_dynamics.test_invariants_of_the_linear_schemes (relative to E_0)"""
    md = _modal(kind, op)
    om, V = md["newmark"]
    dt, steps = md["dt"], 64
    damping = _mode_damping(md, "newmark", part)
    u0, v0 = V[:, 0], 0.5 * om[1] * V[:, 1]
    prob = _problem(oracle, kind, op)
    Cm = dmp.damping_matrix(prob, np.zeros(prob.n), *damping)
    ti = _integrator("newmark", _assembler(engine, kind, op), kind, dt, damping, newton_tol=1e-12 * md["Kphi"])
    ti.set_state(u0, v0)
    E, vs = [0.5 * float(v0 @ (prob.mass() @ v0)) + prob.energy(u0)], [v0]
    for _ in range(steps):
        rec = ti.step(1)
        E.append(rec.kinetic[-1] + rec.stored[-1])
        vs.append(ti.state()[1])
    E = np.array(E)
    bound = 10.0 * steps * _kappa(md, "newmark", dt, *damping) * 1e-12
    work = np.array([dt * float(0.5 * (vs[n] + vs[n + 1]) @ (Cm @ (0.5 * (vs[n] + vs[n + 1])))) for n in range(steps)])
    rise = np.max(np.diff(E)) / E[0]
    defect = np.abs(np.diff(E) + work).max() / E[0]
    print(f"{kind} {op} {part}: E_64 / E_0 = {E[-1] / E[0]:.4f}, largest rise {rise:.3e}, balance defect {defect:.3e} (bound {bound:.3e})")
    assert rise <= bound and defect <= bound and E[-1] < E[0] * (1.0 - 1e-6)


@pytest.mark.gpu
def test_central_differences_bounded_below_the_damped_limit(engine):
    """Hex8 3^3, eta_k with xi = 0.5 at the highest mode: 500 steps at 0.9 dt_crit from a state with every mode in it stay bounded (the
    energy of the last record is below that of the first), where 0.9 of the undamped limit 2 / omega_max, 1.46 dt_crit, is unstable;
    stable_dt returns exactly (2 / om)(sqrt(1 + xi^2) - xi) of its own om"""
    kind, op = "HEX8", "elastic"
    md = _modal(kind, op)
    eta_k = 2.0 * 0.5 / md["om_max"]
    dtc = dmp.dt_crit(md["om_max"], eta_k)
    assert 0.9 * 2.0 / md["om_max"] > 1.4 * dtc
    asm = _assembler(engine, kind, op)
    ti = _integrator("central", asm, kind, 0.9 * dtc, (0.0, eta_k))
    om_dev, dt_dev = ti.stable_dt(30)
    assert dt_dev == dmp.dt_crit(om_dev, eta_k) and om_dev <= md["om_max"] * (1.0 + 1e-10)
    t0 = _integrator("central", asm, kind, 0.9 * dtc, None)
    om0, dt0 = t0.stable_dt(30)
    assert om0 == om_dev and dt0 == 2.0 / om0
    t0.close()
    n = len(md["top"][1])
    u0 = 1e-3 * np.random.default_rng(3).standard_normal(n)
    for k in range(3):
        u0[3 * _clamp(_mesh(kind)[0]) + k] = 0.0
    ti.set_state(u0)
    rec = ti.step(500, record_every=50)
    E = rec.kinetic + rec.stored
    print(f"0.9 dt_crit, xi = 0.5: E over the records {E[0]:.3e} -> {E[-1]:.3e}")
    assert np.isfinite(E).all() and E[-1] < E[0] and np.abs(ti.state()[0]).max() <= np.abs(u0).max()


# ------------------------------------------------------------------------------------------ 6. bits
def _run_cut(engine, scheme, cut, damping, kind="HEX8", op="neo_hookean", tiles=True):
    dt = _dt(kind)
    f, lf = _body_load(kind, LOAD[kind]), _ramp()
    if not tiles:
        engine.set_option("FENRIS_HIP_NO_VECTOR_TILES", "1")
    ti = _integrator(scheme, _assembler(engine, kind, op), kind, dt, damping, f, lf, newton_tol=_newton_tol(f, dt, scheme))
    ti.set_state(np.zeros_like(f))
    steps = 24 if scheme == "central" else 6
    if cut == "one":
        rec = ti.step(steps)
    elif cut == "three":
        for _ in range(3):
            rec = ti.step(steps // 3)
    else:
        rec = ti.step(steps, record_every=5)
    u, v, a, time, step = ti.state()
    assert step == steps
    ti.close()
    if not tiles:
        engine.set_option("FENRIS_HIP_NO_VECTOR_TILES", None)
    return u, v, a, _records(rec)[-1], time


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", SCHEMES)
def test_damped_runs_repeat_and_restart_bit_for_bit(engine, scheme):
    """the scheme of test_dynamics.test_runs_repeat_and_restart_bit_for_bit with damping: two identical runs, and one run cut three ways,
    give identical bits in u, v, a and the final record; eta_k > 0 only where the scheme takes it with a nonlinear operator"""
    dt = _dt("HEX8")
    damping = _damping_for(dt, "both" if scheme == "central" else "mass")
    base = _run_cut(engine, scheme, "one", damping)
    assert np.isfinite(base[0]).all() and np.abs(base[0]).max() > 0
    for cut in ("one", "three", "records"):
        other = _run_cut(engine, scheme, cut, damping)
        for name, p, q in zip(("u", "v", "a", "record", "time"), base, other):
            assert np.array_equal(np.asarray(p), np.asarray(q)), (scheme, cut, name)
    # ... and the damping is not a no-op
    assert not np.array_equal(base[0], _run_cut(engine, scheme, "one", None)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", SCHEMES)
def test_zero_damping_gives_the_bits_of_an_untold_handle(engine, scheme):
    """set_damping(0, 0) -- and a damping set and taken back -- against a handle that was never told"""
    base = _run_cut(engine, scheme, "records", None)
    zero = _run_cut(engine, scheme, "records", (0.0, 0.0))
    for name, p, q in zip(("u", "v", "a", "record", "time"), base, zero):
        assert np.array_equal(np.asarray(p), np.asarray(q)), (scheme, name)
    kind = "HEX8"
    dt = _dt(kind)
    f, lf = _body_load(kind, LOAD[kind]), _ramp()
    ti = _integrator(scheme, _assembler(engine, kind, "neo_hookean"), kind, dt, _damping_for(dt, "mass"), f, lf, newton_tol=_newton_tol(f, dt, scheme))
    ti.set_state(np.zeros_like(f))
    ti.with_damping(0.0, 0.0)
    rec = ti.step(24 if scheme == "central" else 6, record_every=5)
    for name, p, q in zip(("u", "v", "a"), base, ti.state()[:3]):
        assert np.array_equal(p, q), (scheme, name)
    assert np.array_equal(base[3], _records(rec)[-1])


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", SCHEMES)
def test_dirichlet_entries_come_back_bit_for_bit(engine, scheme):
    kind = "HEX8_2"
    m = _mesh(kind)[0]
    dt = _dt(kind)
    f = _body_load(kind, 1e5)
    clamp = _clamp(m)
    rng = np.random.default_rng(5)
    u0, v0 = np.zeros_like(f), 1e-3 * rng.standard_normal(len(f))
    for k in range(3):
        u0[3 * clamp + k] = 1e-3 * rng.standard_normal(len(clamp))   # inhomogeneous values, held
    ti = _integrator(scheme, _assembler(engine, kind, "elastic"), kind, dt, _damping_for(dt, "both"), f, newton_tol=_newton_tol(f, dt, scheme))
    ti.set_state(u0, v0)
    ti.step(5, record_every=2)
    u, v, a, _, _ = ti.state()
    free = np.ones(len(f), dtype=bool)
    for k in range(3):
        assert np.array_equal(u[3 * clamp + k], u0[3 * clamp + k])
        assert not v[3 * clamp + k].any() and not a[3 * clamp + k].any()
        free[3 * clamp + k] = False
    assert np.abs(u[free] - u0[free]).max() > 0 and np.isfinite(u).all()


TILE_TOLERANCE = {
    'elastic': (8.2e-14, 0.0e+00, 1.6e-12),
    'neo_hookean': (6.3e-14, 0.0e+00, 1.3e-12),
}


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["elastic", "neo_hookean"])
def test_two_tiles_agree_with_the_route_off_the_tiles(engine, oracle, op):
    """Hex8 7^3 (two tiles: node sums cross a tile boundary), central differences with both coefficients: the fused route against the same
    run with the tiles switched off (the ordered per-element route), within the tolerance of the trajectory test, measured the same way"""
    kind = "HEX8_7"
    dt = _dt(kind)
    damping = _damping_for(dt, "both")
    f, lf = _body_load(kind, LOAD[kind]), _ramp()
    _, d_perm, d_newton, tol = _measured_tolerance(oracle, kind, op, "central", f, lf, dt, damping, 0.0)
    tol = _check_constants(op, d_perm, d_newton, tol, TILE_TOLERANCE)
    runs = {}
    for tiles in (True, False):
        if not tiles:
            engine.set_option("FENRIS_HIP_NO_VECTOR_TILES", "1")
        ti = _integrator("central", _assembler(engine, kind, op), kind, dt, damping, f, lf)
        runs[tiles] = _device_run(ti, len(f))
        ti.close()
        t2 = _integrator("central", _assembler(engine, kind, op), kind, dt, damping, f, lf)
        t2.set_state(np.zeros(len(f)))
        t2.state()
        assert engine.last_kernel_name() == ("k_damped_pass_tiled + k_dynamics_from_partials" if tiles
                                             else "k_residual_elements + k_vector_from_elements_soa + k_dynamics_update"), engine.last_kernel_name()
        t2.close()
        if not tiles:
            engine.set_option("FENRIS_HIP_NO_VECTOR_TILES", None)
    _assert_parity(runs[True], runs[False], tol, f"{kind} {op} tiles against no tiles")


# ------------------------------------------------------------------------------------------ 7. codes
@pytest.mark.gpu
def test_damping_codes(engine):
    lib = engine._lib
    kind = "HEX8_2"
    dt = _dt(kind)
    f = _body_load(kind, 1e5)
    n = len(f)
    ti = _integrator("newmark", _assembler(engine, kind, "neo_hookean"), kind, dt, None, f, newton_tol=_newton_tol(f, dt, "newmark"))
    h = ti._handle()
    for bad in ((-1.0, 0.0), (0.0, -1e-9), (float("nan"), 0.0), (0.0, float("nan")), (float("inf"), 0.0), (0.0, float("inf"))):
        assert lib.fh_dynamics_set_damping(h, *bad) == FH_BAD_ARGUMENT, bad
        with pytest.raises(fa.FenrisError) as e:
            ti.with_damping(*bad)
        assert e.value.code == FH_BAD_ARGUMENT
    ti._damping = None
    assert ti.damping() == fa.RayleighDamping(0.0, 0.0)   # a refused call leaves the coefficients
    m, k = C.c_double(7.0), C.c_double(7.0)
    assert lib.fh_dynamics_set_damping(h, 2.0, 3.0) == 0 and lib.fh_dynamics_damping(h, C.byref(m), None) == 0 and m.value == 2.0
    assert lib.fh_dynamics_damping(h, None, C.byref(k)) == 0 and k.value == 3.0
    assert lib.fh_dynamics_set_damping(None, 0.0, 0.0) == FH_BAD_ARGUMENT and lib.fh_dynamics_damping(None, None, None) == FH_BAD_ARGUMENT
    # eta_k > 0 + implicit + nonlinear: FH_UNSUPPORTED, the state untouched
    rng = np.random.default_rng(2)
    u0, v0 = 1e-4 * rng.standard_normal(n), 1e-3 * rng.standard_normal(n)
    ti.with_damping(0.0, 0.0)
    ti.set_state(u0, v0)
    u0, v0 = ti.state()[:2]   # (v with the clamped entries zero)
    for scheme_ti in (ti, _integrator("euler", ti.element_assembler, kind, dt, None, f, newton_tol=_newton_tol(f, dt, "euler"))):
        scheme_ti.set_state(u0, v0)
        scheme_ti.with_damping(0.1 / dt, 0.2 * dt)
        with pytest.raises(fa.DynamicsError) as e:
            scheme_ti.step(3)
        assert e.value.code == FH_UNSUPPORTED and e.value.steps_done == 0 and "stiffness damping" in e.value.message
        u, v = np.zeros(n), np.zeros(n)
        t, s = C.c_double(-1.0), C.c_uint64(9)
        assert lib.fh_dynamics_state(scheme_ti._handle(), _ffi.fp(u), _ffi.fp(v), None, C.byref(t), C.byref(s)) == 0
        assert np.array_equal(u, u0) and np.array_equal(v, v0) and s.value == 0 and t.value == 0.0
        scheme_ti.with_damping(0.1 / dt, 0.0)   # eta_m alone works with every material
        assert scheme_ti.step(2).steps_done == 2
    # a first-order handle
    fo = fa.ForwardEuler(ti.element_assembler, RHO, 1e-6).with_dirichlet_nodes(_clamp(_mesh(kind)[0]))
    with pytest.raises(TypeError):
        fo.with_damping(1.0, 0.0)
    hf = fo._handle()
    assert lib.fh_dynamics_set_damping(hf, 1.0, 0.0) == FH_BAD_ARGUMENT and "first-order" in engine.last_error()
    assert lib.fh_dynamics_set_damping(hf, 0.0, 0.0) == FH_BAD_ARGUMENT and lib.fh_dynamics_damping(hf, C.byref(m), C.byref(k)) == FH_BAD_ARGUMENT


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["central", "newmark"])
def test_changing_the_coefficients_forms_a_n_again(engine, oracle, scheme):
    """a_n of a state with v != 0 follows the coefficients: after every change fh_dynamics_state returns the a_0 of the reference for the
    pair now set, and the residual evaluations of the next step count the one that formed it"""
    kind, op = "TET4", "elastic"
    dt = _dt(kind)
    f = _body_load(kind, 1e5)
    prob = _problem(oracle, kind, op, f)
    rng = np.random.default_rng(4)
    u0, v0 = 1e-4 * rng.standard_normal(len(f)), 1e-2 * rng.standard_normal(len(f))
    ti = _integrator(scheme, _assembler(engine, kind, op), kind, dt, None, f, newton_tol=_newton_tol(f, dt, scheme))
    ti.set_state(u0, v0)
    seen = []
    for damping in ((0.0, 0.0), (0.1 / dt, 0.0), (0.1 / dt, 0.2 * dt), (0.0, 0.2 * dt), (0.0, 0.0)):
        ti.with_damping(*damping)
        a = ti.state()[2]
        want = _reference_run(prob, scheme, u0, v0, dt, 0, 0, damping)[2] if scheme == "central" else \
            dmp.implicit(prob, scheme, u0, v0, dt, 0, damping[0], damping[1])[3]
        err = np.abs(a - want).max() / np.abs(want).max()
        print(f"{scheme} {damping}: a_0 against the reference {err:.3e}")
        assert err <= 1e-9
        seen.append(a)
    assert np.array_equal(seen[0], seen[-1]) and not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    if scheme == "central":   # (one residual evaluation per step, and one more where a_n is formed)
        ti.with_damping(0.1 / dt, 0.0)
        first = ti.step(1).stats[1]
        again = ti.step(1).stats[1]
        ti.with_damping(0.2 / dt, 0.0)
        changed = ti.step(1).stats[1]
        assert (first, again, changed) == (2, 1, 2)
