"""Obstacles that translate along piecewise-linear paths (fh_set_obstacle_paths, fh_set_obstacle_time), the relative slip of the friction
term against them, the integrators' contact clock and the force resultants per obstacle (fh_contact_resultants), against the NumPy
statement of tests/motion_reference.py.

Tolerances.  The bitwise statements are bitwise.  Every comparison with the reference is held to a tolerance measured from the reference
alone, the method of tests/test_damping.py.  Trajectories (motion_reference.measured_tolerance): d_perm from a run of the reference on a
permuted connectivity, d_newton (implicit schemes) from a Newton tolerance 100 times smaller, tolerance 20 (d_perm + d_newton), floored at
1e-13.  The node term (motion_reference.measured_term_tolerance) reads no connectivity and solves nothing, which leaves the floor, 1e-13 of
the largest entry; what the reference can do two ways is take the lag obstacle at point + d(t_lag) or at (point + d(t)) - c_o, and d_perm
is the difference of the two.  TERM_TOLERANCE and TRAJECTORY_TOLERANCE hold what the CPU measured; every test measures again and asserts
that it stays within a factor 10.

No launch is added per step: besides the residual count of the records (stats), fh_last_kernel_name of a central-difference launch with
paths set is checked to be the element pass and the fused node pass on the tiles, and the composed route with one k_contact_force off them.

Conditions on the inputs are asserted on the reference, never on the device result: in every trajectory some node is in contact with a
moving obstacle at 4 or more of the 16 steps; in every friction case at least one node-step sticks (|s| < eps) and one slides."""
import functools
import os

import numpy as np
import pytest

import fenris_amd as fa
from fenris_amd import _ffi, quadrature

import contact_reference as cr
import dynamics_reference as dr
import friction_reference as fr
import motion_reference as mr

LAME = fa.LameParameters(384.0, 577.0)
RHO = 1.0
FH_BAD_ARGUMENT, FH_INVALID_STATE, FH_UNSUPPORTED = 2, 5, 6
OKIND = {"QUAD4": 0, "HEX8": 1, "TET4": 2, "HEX27": 3, "TRI3": 4}
NEW = ("fh_set_obstacle_paths", "fh_set_obstacle_time", "fh_obstacle_offsets", "fh_obstacle_count", "fh_contact_resultants", "fh_dynamics_set_boundary_motion",
       "fh_dynamics_set_boundary_motion_dev")
SHORT_SUM = 1e-13
EPS = 2.0 ** -7
STEPS, EVERY = 16, 4
KINDS = ("HEX8", "TET4", "QUAD4", "TRI3", "HEX8_776", "HEX27")


@pytest.fixture()
def engine():
    eng = fa.Engine(0)
    yield eng
    eng.close()


# ------------------------------------------------------------------------------------------ meshes, problems, integrators
@functools.lru_cache(maxsize=None)
def _mesh(kind):
    P, T, Q = fa.procedural, quadrature.tensor, quadrature.total_order
    make = {"HEX8": (lambda: P.create_unit_box_uniform_hex_mesh_3d(3), T.hexahedron_gauss(2)),
            "TET4": (lambda: P.create_unit_box_uniform_tet_mesh_3d(2), Q.tetrahedron(2)),
            "QUAD4": (lambda: P.create_unit_square_uniform_quad_mesh_2d(4), T.quadrilateral_gauss(2)),
            "TRI3": (lambda: P.create_unit_square_uniform_tri_mesh_2d(4), Q.triangle(2)),
            "HEX8_776": (lambda: P.create_rectangular_uniform_hex_mesh(1.0 / 7.0, 7, 7, 6, 1), T.hexahedron_gauss(2)),   # two tiles, two workgroups of nodes
            "HEX27": (lambda: fa.hex27_mesh_from_hex8(P.create_unit_box_uniform_hex_mesh_3d(2)), T.hexahedron_gauss(3))}   # off the tiles
    gen, (w, p) = make[kind]
    return gen(), np.asarray(w), np.asarray(p)


def _okind(kind):
    return OKIND[kind.split("_")[0]]


def _clamp(m):
    x = m.vertices[:, 0]
    return np.where(np.isclose(x, x.min()))[0]


def _problem(oracle, kind, op, f=None, perm=None, obstacles=(), node_weights=None, direct="sparse"):
    """the reference's problem, clamped at x = min; perm: a permutation of the connectivity rows (another summation order, nothing else)"""
    m, w, p = _mesh(kind)
    groups = [(np.asarray(m.connectivity), w, p)]
    if perm is not None:
        groups = [(c[np.random.default_rng(perm + g).permutation(len(c))], wg, pg) for g, (c, wg, pg) in enumerate(groups)]
    oop = {"elastic": oracle.LINEAR_ELASTIC, "neo_hookean": oracle.NEO_HOOKEAN}[op]
    return cr.ContactProblem(oracle, _okind(kind), oop, m.vertices, groups, params=LAME.as_pair(), rho=RHO, dirichlet=_clamp(m), f=f,
                             direct=direct, obstacles=obstacles, node_weights=node_weights)


def _operator(op):
    return fa.MaterialEllipticOperator({"elastic": fa.LinearElasticMaterial, "neo_hookean": fa.NeoHookeanMaterial}[op]())


def _assembler(engine, kind, op, u=None):
    m, w, p = _mesh(kind)
    qt = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(LAME)
    return (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(m).with_operator(_operator(op)).with_quadrature_table(qt)
            .with_u(np.zeros(m.vertices.size) if u is None else u).build())


def _integrator(scheme, asm, kind, dt, newton_tol=1e-8, f=None):
    if scheme == "central":
        ti = fa.CentralDifference(asm, RHO, dt)
    else:
        ti = fa.Newmark(asm, RHO, dt) if scheme == "newmark" else fa.BackwardEuler(asm, RHO, dt)
        ti.with_newton(fa.NewtonSettings(60, newton_tol), linear_rel_tol=1e-14)
    return ti.with_dirichlet_nodes(_clamp(_mesh(kind)[0])).with_load(f)


@functools.lru_cache(maxsize=None)
def _modal(kind):
    """dt = 1 / omega_max of the clamped linear-elastic body on its lumped mass, and the smallest lumped mass of a free dof"""
    from oracle import oracle as o

    o.lib()
    prob = _problem(o, kind, "elastic", direct="dense")
    wl, _ = dr.dense_pencil(prob, np.zeros(prob.n), True)
    return {"dt": 1.0 / np.sqrt(wl[-1]), "om_max": np.sqrt(wl[-1]), "m_min": prob.lumped()[prob.free].min()}


def _fa_obstacles(obstacles, mu=None, paths=None, node_weights=None, **kw):
    out = []
    for j, (kind, p, q, k) in enumerate(obstacles):
        cls = fa.HalfSpace if kind == "half_space" else fa.Ball if kind == "ball" else fa.Cavity
        path = None if paths is None or paths[j] is None else fa.ObstaclePath(*paths[j])
        out.append(cls(p, q, k, friction=0.0 if mu is None else mu[j], path=path))
    return fa.Obstacles(out, node_weights, **kw)


def _records(rec):
    return np.stack([rec.kinetic, rec.stored, rec.load_potential, rec.time], axis=1)


def _rel(x, y):
    return np.abs(np.asarray(x) - np.asarray(y)).max() / max(np.abs(np.asarray(y)).max(), 1e-300)


def _check(name, err, tol):
    print(f"{name}: {err:.3e} (bound {tol:.3e})")
    assert err <= tol, (name, err, tol)


def _code(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except fa.FenrisError as e:
        return e.code
    return 0


# ------------------------------------------------------------------------------------------ the scene of the term tests
def _term_scene(kind):
    """three obstacles of the three kinds with a path each and a fourth, a half-space, without one; node weights, a lag state and a u with
    slips on both sides of eps; the clock (t, t_lag) inside two different segments"""
    X = np.asarray(_mesh(kind)[0].vertices)
    N, d = X.shape
    rng = np.random.default_rng(31)
    obstacles = [("half_space", (0.0,) * (d - 1) + (0.25,), (0.0,) * (d - 1) + (1.0,), 1.0e4), ("ball", (1.1,) * d, 0.7, 2.0e3),
                 ("cavity", (0.4, 0.5, 0.6)[:d], 0.75 if d == 3 else 0.6, 5.0e3), ("half_space", (0.3,) * d, (1.0, 2.0, 3.0)[:d], 1.0e4)]
    paths = [([0.0, 1.0, 2.0], [[0.0] * d, [0.125, 0.0625, 0.03125][:d], [0.25, -0.0625, 0.0625][:d]]),
             ([0.5, 1.5], [[0.0] * d, [-0.0625] * d]),
             ([0.0, 2.0], [[0.0] * d, [0.03125, -0.015625, 0.0078125][:d]]), None]
    mu = [0.5, 0.3, 0.7, 0.2]
    w = rng.uniform(0.5, 2.0, N)
    ubar = rng.uniform(-0.02, 0.02, N * d)
    u = ubar + (rng.uniform(-0.02, 0.02, (N, d)) * rng.choice([0.1, 1.0], (N, 1))).reshape(-1)
    return obstacles, paths, mu, w, ubar, u, (1.25, 0.75)


def _set_scene(engine, kind, friction=True, clock=True):
    obs, paths, mu, w, ubar, u, (t, t_lag) = _term_scene(kind)
    engine.set_obstacles(_fa_obstacles(obs, mu if friction else None, paths, w, slip_length=EPS))
    if friction:
        engine._check(engine._lib.fh_set_friction_reference(engine._h, _ffi.fp(np.ascontiguousarray(ubar))))
    if clock:
        engine.set_obstacle_time(t, t_lag)


def _csr_added(engine, asm):
    k = fa.CsrAssembler(fa.SCATTER_GATHER).assemble(asm)
    vals = np.zeros_like(k.values)
    fa.Contact(engine).add_tangent_to(vals)
    return fa.CsrMatrix(k.row_offsets, k.col_indices, vals).to_scipy().toarray()


# measured on the CPU with the reference alone (mr.measured_term_tolerance): d_perm (the lag obstacle taken both ways), no d_newton, and
# the tolerance 20 d_perm, floored at 1e-13
TERM_TOLERANCE = {
    ('HEX8', 'slip'): (0.0e+00, 0.0e+00, 1.0e-13),
    ('HEX8', 'resultants', False): (0.0e+00, 0.0e+00, 1.0e-13),
    ('HEX8', 'resultants', True): (0.0e+00, 0.0e+00, 1.0e-13),
    ('QUAD4', 'slip'): (0.0e+00, 0.0e+00, 1.0e-13),
    ('QUAD4', 'resultants', False): (0.0e+00, 0.0e+00, 1.0e-13),
    ('QUAD4', 'resultants', True): (0.0e+00, 0.0e+00, 1.0e-13),
    ('HEX8_776', 'slip'): (0.0e+00, 0.0e+00, 1.0e-13),
    ('HEX8_776', 'resultants', False): (0.0e+00, 0.0e+00, 1.0e-13),
    ('HEX8_776', 'resultants', True): (0.0e+00, 0.0e+00, 1.0e-13),
    ('HEX27', 'slip'): (0.0e+00, 0.0e+00, 1.0e-13),
}


# ------------------------------------------------------------------------------------------ no GPU: declarations, the path formula, the reference
def test_entry_points_are_declared_exported_and_bound():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "fenris_hip.h")).read()
    rs = open(os.path.join(root, "bindings", "fenris_hip_sys.rs")).read()
    for name in NEW:
        assert name in _ffi.exported_symbols() and name + "(" in hdr and "fn " + name + "(" in rs
    assert callable(fa.Contact.resultants) and callable(fa.Contact.obstacle_offsets) and callable(fa.Engine.set_obstacle_time)
    assert callable(fa.TimeIntegrator.with_boundary_motion)
    with pytest.raises(TypeError):
        fa.FirstOrderIntegrator.with_boundary_motion(None, np.zeros(3), [0.0, 1.0])
    path = fa.ObstaclePath([0.0, 1.0], [[0.0, 0.0], [1.0, 2.0]])
    assert fa.Ball((0, 0, 0), 1.0, 1.0, path=path).path is path and fa.HalfSpace((0, 0, 0), (0, 0, 1), 1.0).path is None
    assert fa.Obstacles([fa.Cavity((0, 0, 0), 1.0, 1.0, path=path)]).has_paths() and not fa.Obstacles([fa.Cavity((0, 0, 0), 1.0, 1.0)]).has_paths()
    with pytest.raises(ValueError):
        fa.ObstaclePath([0.0, 0.0], [[0.0, 0.0], [1.0, 2.0]])       # not strictly increasing
    with pytest.raises(TypeError):
        fa.Ball((0, 0, 0), 1.0, 1.0, path=([0.0], [[0.0, 0.0, 0.0]]))


def test_obstacle_path_offset_is_the_reference_formula():
    """at the knots, inside the segments, before the first and after the last knot, and for a one-knot path: the same bits"""
    rng = np.random.default_rng(2)
    times = np.cumsum(rng.uniform(0.1, 1.0, 6))
    offsets = rng.uniform(-1.0, 1.0, (6, 3))
    path = fa.ObstaclePath(times, offsets)
    ts = list(times) + list(0.5 * (times[1:] + times[:-1])) + list(rng.uniform(times[0], times[-1], 40)) + [times[0] - 1.0, times[-1] + 1.0,
                                                                                                             np.nextafter(times[2], 0.0), np.nextafter(times[2], 9.0)]
    for t in ts:
        assert np.array_equal(path.offset(t), mr.path_offset((times, offsets), t)), t
    for k, t in enumerate(times):
        assert np.array_equal(path.offset(t), offsets[k])
    assert np.array_equal(path.offset(times[0] - 1.0), offsets[0]) and np.array_equal(path.offset(times[-1] + 1.0), offsets[-1])
    one = fa.ObstaclePath([0.5], [[1.0, 2.0]])
    for t in (0.0, 0.5, 1.0):
        assert np.array_equal(one.offset(t), [1.0, 2.0, 0.0]) and np.array_equal(mr.path_offset(([0.5], [[1.0, 2.0]]), t), [1.0, 2.0, 0.0])
    assert not mr.path_offset(None, 1.0).any() and not fa.ObstaclePath([], []).offset(1.0).any()
    cv = fa.ObstaclePath.constant_velocity((1.0, -2.0, 0.5), 4.0)
    assert np.array_equal(cv.offset(1.0), [1.0, -2.0, 0.5]) and np.array_equal(cv.offset(9.0), [4.0, -8.0, 2.0])


@pytest.mark.parametrize("d", [2, 3])
def test_reference_is_galilean(d):
    """shifting every slip and the obstacle's displacement by one vector changes neither q nor D, up to the cancellation in d - c:
    an error 2^-53 |shift| in the slip, against a force whose slope in the slip is at most 2 mu lam / eps, summed over the components and
    the projection: 16 * 2^-52 |shift| / eps with |shift| <= 0.5 sqrt(3); and a node that moves with the obstacle feels nothing"""
    _check(f"{d}-D galilean", mr.galilean_check(d), 16.0 * 2.0 ** -52 * 0.5 * np.sqrt(3.0) / EPS)


# ------------------------------------------------------------------------------------------ GPU 1: moved equals placed
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["HEX8", "QUAD4"])
def test_moved_obstacles_equal_placed_obstacles(kind):
    """paths and a clock against a second engine whose obstacles are constructed at point + d_o(t): energy, force, gap, the tangent's map
    and diagonal and the CSR blocks, bit for bit; fh_obstacle_offsets returns d_o(t) and d_o(t_lag) to the bit"""
    obs, paths, mu, w, ubar, u, (t, t_lag) = _term_scene(kind)
    n = len(u)
    d = n // len(w)
    x = np.random.default_rng(8).uniform(-1.0, 1.0, n)

    def pieces(moved):
        eng = fa.Engine(0)
        try:
            asm = _assembler(eng, kind, "elastic", u)
            if moved:
                eng.set_obstacles(_fa_obstacles(obs, None, paths, w))
                eng.set_obstacle_time(t, t_lag)
                cur, lag = fa.Contact(eng).obstacle_offsets()
                for o, q in enumerate(paths):
                    assert np.array_equal(cur[o], mr.path_offset(q, t)[:d]) and np.array_equal(lag[o], mr.path_offset(q, t_lag)[:d])
            else:
                eng.set_obstacles(_fa_obstacles(mr.placed(obs, paths, t), None, None, w))
            con = fa.Contact(eng)
            tan = fa.MatrixFreeTangent(asm)     # (owns no obstacles: the engine's stay)
            return [np.array([con.energy()]), con.force(), con.gap(), tan.apply(np.zeros(n), x).copy(), tan.diagonal(), _csr_added(eng, asm)]
        finally:
            eng.close()

    a, b = pieces(True), pieces(False)
    assert np.abs(a[1]).max() > 0.0 and (a[2] < 0.0).any()
    X = np.asarray(_mesh(kind)[0].vertices)
    assert not np.array_equal(cr.force(mr.placed(obs, paths, t), X, u, w), cr.force(obs, X, u, w))     # the paths matter here
    for i, (p, q) in enumerate(zip(a, b)):
        assert np.array_equal(p, q), i


# ------------------------------------------------------------------------------------------ GPU 2: the relative slip
@pytest.mark.gpu
@pytest.mark.parametrize("kind,route", [("HEX8", "tiles"), ("QUAD4", "tiles"), ("HEX8_776", "tiles"), ("HEX27", "off")])
def test_relative_slip_parity(engine, kind, route):
    """t != t_lag: the friction force, potential, CSR blocks, tangent map and diagonal against the reference at the measured tolerance (the
    library shifts the current point back by c_o, the reference places the obstacle at point + d_o(t_lag): the reference does both for d_perm)"""
    obs, paths, mu, w, ubar, u, (t, t_lag) = _term_scene(kind)
    X = np.asarray(_mesh(kind)[0].vertices)
    N, d = X.shape
    n = X.size
    cur, lag, c = mr.placed(obs, paths, t), mr.placed(obs, paths, t_lag), mr.displacements(paths, t, t_lag)
    ys = mr.slips(lag, mu, X, ubar, u - ubar, c, w)
    assert min(ys) < EPS <= max(ys) and len(ys) >= 10 and max(np.abs(ci).max() for ci in c) > 0.01
    assert _rel(mr.friction_force(lag, mu, X, ubar, u - ubar, c, EPS, w), fr.force(obs, mu, X, ubar, u - ubar, EPS, w)) > 1e-3     # c_o matters
    asm = _assembler(engine, kind, "elastic", u)
    _set_scene(engine, kind)
    con = fa.Contact(engine)

    def reference(perm):
        at = lag if perm is None else mr.shifted_back(cur, c)
        args = (at, mu, X, ubar, u - ubar, c, EPS, w)
        return [mr.friction_force(*args), np.array([mr.friction_potential(*args)]), mr.friction_tangent(*args).toarray(), mr.friction_blocks(*args)]

    (q_ref, D_ref, H_ref, Hb_ref), d_perm, d_newton, bound = mr.measured_term_tolerance(reference)
    bound = mr.check_constants(TERM_TOLERANCE, (kind, "slip"), d_perm, d_newton, bound)
    D_ref = float(D_ref[0])
    B_ref = cr.tangent(cur, X, u, w, exact=False).toarray()
    _check(f"{kind} friction force", _rel(con.friction_force(), q_ref), bound)
    _check(f"{kind} potential", abs(con.friction_potential() - D_ref) / D_ref, bound)
    _check(f"{kind} contact force at the current position", _rel(con.force(), cr.force(cur, X, u, w)), bound)
    K = _csr_added(engine, asm)
    _check(f"{kind} csr blocks B + H", np.abs(K - (B_ref + H_ref)).max() / np.abs(B_ref + H_ref).max(), bound)
    assert np.array_equal(K, K.T)                                   # symmetric to the bit
    blocks = cr.blocks(cur, X, u, w) + Hb_ref                       # ... and the blocks are blocks()
    got = np.array([K[d * i:d * i + d, d * i:d * i + d] for i in range(N)])
    _check(f"{kind} csr blocks against blocks()", np.abs(got - blocks).max() / np.abs(blocks).max(), bound)
    x = np.random.default_rng(6).uniform(-1.0, 1.0, n)
    obstacles = _fa_obstacles(obs, mu, paths, w, slip_length=EPS)
    tan = fa.MatrixFreeTangent(asm).with_obstacles(obstacles).with_friction_reference(ubar)
    engine.set_obstacle_time(t, t_lag)
    y1 = tan.apply(np.zeros(n), x).copy()
    name = engine.last_kernel_name()
    d1 = tan.diagonal()
    tan0 = fa.MatrixFreeTangent(asm).with_obstacles(_fa_obstacles(obs, None, paths, w))
    engine.set_obstacle_time(t, t_lag)
    y0, d0 = tan0.apply(np.zeros(n), x).copy(), tan0.diagonal()
    Hx = H_ref @ x
    _check(f"{kind} apply difference", np.abs((y1 - y0) - Hx).max() / max(np.abs(Hx).max(), np.abs(y0).max()), bound)
    _check(f"{kind} diagonal difference", np.abs((d1 - d0) - H_ref.diagonal()).max() / np.abs(d1).max(), bound)
    if route == "tiles":
        assert name.endswith("k_operator_from_partials") and "k_contact_apply" not in name, name
    else:
        assert name.endswith("+ k_contact_apply"), name


@pytest.mark.gpu
def test_the_clock_returns_with_obstacles_that_are_bound_again(engine):
    """the quasi-static recipe: a tangent's obstacles and clock, another object takes the engine (its own obstacles, clock (0, 0)), the
    first is used again: its obstacles go back to the engine with the clock it was given, and the map repeats bit for bit"""
    kind = "HEX8"
    obs, paths, mu, w, ubar, u, (t, t_lag) = _term_scene(kind)
    n = len(u)
    x = np.random.default_rng(6).uniform(-1.0, 1.0, n)
    asm = _assembler(engine, kind, "elastic", u)
    tan = fa.MatrixFreeTangent(asm).with_obstacles(_fa_obstacles(obs, mu, paths, w, slip_length=EPS)).with_friction_reference(ubar)
    engine.set_obstacle_time(t, t_lag)
    con = fa.Contact(engine)
    y1, off1 = tan.apply(np.zeros(n), x).copy(), con.obstacle_offsets()
    assert off1[0].any() and not np.array_equal(off1[0], off1[1])
    other = fa.MatrixFreeTangent(asm).with_obstacles(_fa_obstacles(obs[:2], None, paths[:2], w))
    other.apply(np.zeros(n), x)
    assert con.obstacle_offsets()[0].shape == (2, 3) and not con.obstacle_offsets()[0].any()
    y2, off2 = tan.apply(np.zeros(n), x).copy(), con.obstacle_offsets()
    assert np.array_equal(off1[0], off2[0]) and np.array_equal(off1[1], off2[1]) and np.array_equal(y1, y2)


# ------------------------------------------------------------------------------------------ GPU 3: co-moving gives no friction
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["HEX8", "QUAD4"])
def test_a_node_that_moves_with_the_obstacle_feels_no_friction(engine, kind):
    """a half-space moves tangentially by c and u - ubar = c on every node, all exactly representable: the friction force is exactly zero
    and the potential is sum mu lam eps / 3 (a short sum: 1e-13)"""
    X = np.asarray(_mesh(kind)[0].vertices)
    N, d = X.shape
    normal = (0.0,) * (d - 1) + (1.0,)
    floor = [("half_space", (0.0,) * (d - 1) + (0.3,), normal, 1.0e4)]
    c = np.zeros(3)
    c[0] = 2.0 ** -4
    if d == 3:
        c[1] = -2.0 ** -5
    paths = [([0.0, 1.0], [np.zeros(3), 2.0 * c])]            # d(0.5) = c exactly
    ubar = np.zeros((N, d))
    ubar[:, 0] = 2.0 ** -6
    u = ubar + c[:d]
    _assembler(engine, kind, "elastic", u.reshape(-1))
    engine.set_obstacles(_fa_obstacles(floor, [0.5], paths, None, slip_length=EPS))
    engine._check(engine._lib.fh_set_friction_reference(engine._h, _ffi.fp(np.ascontiguousarray(ubar.reshape(-1)))))
    con = fa.Contact(engine)
    assert con.friction_force().any()                              # the clock is (0, 0): the obstacle has not moved, the nodes have
    engine.set_obstacle_time(0.5, 0.0)
    cur, lag = con.obstacle_offsets()
    assert np.array_equal(cur[0], c[:d]) and not lag.any()
    assert not con.friction_force().any()
    lam = sum(ml for _, _, ml, _, _, _ in mr._visit(floor, [0.5], X, ubar.reshape(-1), np.zeros((N, d)), [np.zeros(3)], None))
    assert lam > 0.0
    _check(f"{kind} potential of no slip", abs(con.friction_potential() - lam * EPS / 3.0) / (lam * EPS / 3.0), SHORT_SUM)
    R, Q = con.resultants()
    assert not Q.any() and R[0, d - 1] < 0.0


# ------------------------------------------------------------------------------------------ GPU 9: the resultants
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["HEX8", "QUAD4", "HEX8_776"])
@pytest.mark.parametrize("friction", [False, True])
def test_resultants_parity(engine, kind, friction):
    """R_o and Q_o against the reference (HEX8, QUAD4: fewer than 256 nodes, one partial row; HEX8_776: 448 nodes, two), sum_o R_o against
    the column sums of Contact.force(), two calls bit for bit, at the measured tolerance relative to the sum of the magnitudes (a sum over
    N <= 448 nodes in a tree errs by N 2^-53 of it at the most, 5e-14: inside the floor)"""
    obs, paths, mu, w, ubar, u, (t, t_lag) = _term_scene(kind)
    X = np.asarray(_mesh(kind)[0].vertices)
    N, d = X.shape
    assert (N < 256) == (kind != "HEX8_776")
    cur, lag, c = mr.placed(obs, paths, t), mr.placed(obs, paths, t_lag), mr.displacements(paths, t, t_lag)
    _assembler(engine, kind, "elastic", u)
    _set_scene(engine, kind, friction)
    con = fa.Contact(engine)
    R, Q = con.resultants()
    assert engine.last_kernel_name() == "k_contact_resultants" and R.shape == Q.shape == (len(obs), d)
    R2, Q2 = con.resultants()
    assert np.array_equal(R, R2) and np.array_equal(Q, Q2)

    def reference(perm):
        if not friction:
            return [mr.resultants(cur, X, u, w)[0]]
        return list(mr.resultants(cur, X, u, w, mu, lag if perm is None else mr.shifted_back(cur, c), ubar, u - ubar, c, EPS))

    ref, d_perm, d_newton, bound = mr.measured_term_tolerance(reference)
    bound = mr.check_constants(TERM_TOLERANCE, (kind, "resultants", friction), d_perm, d_newton, bound)
    R_ref = ref[0]
    if friction:
        Q_ref = ref[1]
        mag_q = max(np.abs(mr.friction_force(lag, mu, X, ubar, u - ubar, c, EPS, w, only=o)).reshape(N, d).sum(axis=0).max() for o in range(len(obs)))
        assert np.abs(Q_ref).max() > 0.0
        _check(f"{kind} Q", np.abs(Q - Q_ref).max() / mag_q, bound)
    else:
        assert not Q.any()
    assert (np.abs(R_ref).max(axis=1) > 0.0).sum() >= 3            # several obstacles carry force
    mag = max(np.abs(cr.force([ob], X, u, w)).reshape(N, d).sum(axis=0).max() for ob in cur)
    _check(f"{kind} R", np.abs(R - R_ref).max() / mag, bound)
    g = con.force().reshape(N, d)
    _check(f"{kind} sum of R against the force", np.abs(R.sum(axis=0) - g.sum(axis=0)).max() / np.abs(g).sum(axis=0).max(), bound)


# ------------------------------------------------------------------------------------------ the scenes of the trajectories
def _scene(kind, which):
    """(obstacles, paths, mu, eps_v).  The last axis is "up".  Stiffnesses are half of m_min omega_max^2, inside the explicit limit at
    dt = 1 / omega_max.  "ball": a ball of radius 1 over the top face, off the clamp, pressed in by 0.05 over six steps, held for four,
    retracted past its start over six.  "belt": the floor under the body, 0.01 into its bottom face, sliding sideways with mu = 0.5, slowly
    (a quarter of the slip velocity: sticking) for eight steps and fast (four times it: sliding) for eight"""
    X = np.asarray(_mesh(kind)[0].vertices)
    d = X.shape[1]
    md = _modal(kind)
    dt, k = md["dt"], 0.5 * md["m_min"] * md["om_max"] ** 2
    if which == "ball":
        centre = [0.625, 0.5, 0.0][:d - 1] + [X[:, d - 1].max() + 1.0]
        down = lambda z: [0.0] * (d - 1) + [z]
        return [("ball", tuple(centre), 1.0, k)], [([0.0, 6 * dt, 10 * dt, 16 * dt], [down(0.0), down(-0.05), down(-0.05), down(0.025)])], None, None
    pen = 0.01
    eps_v = 2.0 * 0.5 * pen / dt          # (2 c dt = 2 mu k pen dt / (eps_v m) <= 1/2 with k / m <= omega_max^2 / 2)
    floor = [("half_space", tuple([0.0] * (d - 1) + [pen]), tuple([0.0] * (d - 1) + [1.0]), k)]
    side = lambda x: [x] + [0.0] * (d - 1)
    x8 = 0.25 * eps_v * 8 * dt
    return floor, [([0.0, 8 * dt, 16 * dt], [side(0.0), side(x8), side(x8 + 4.0 * eps_v * 8 * dt)])], [0.5], eps_v


def _newton_tol(kind, which, scheme):
    """1e-10 of the penalty force scale k * 0.01 times beta dt^2: the reference and the device both stop at rounding level"""
    md = _modal(kind)
    k = 0.5 * md["m_min"] * md["om_max"] ** 2
    return 1e-10 * k * 0.01 * {"central": 0.0, "newmark": 0.25, "euler": 1.0}[scheme] * md["dt"] ** 2


def _reference_trajectory(oracle, kind, op, scheme, which, perm=None, tol=0.0, probe=None):
    obs, paths, mu, eps_v = _scene(kind, which)
    mp = mr.MovingProblem(_problem(oracle, kind, op, perm=perm, obstacles=obs), paths, mu)
    n, dt = mp.n, _modal(kind)["dt"]
    if scheme == "central":
        return mr.central_difference(mp, np.zeros(n), np.zeros(n), dt, STEPS, EVERY, eps_v, probe=probe)
    return mr.implicit(mp, scheme, np.zeros(n), np.zeros(n), dt, STEPS, EVERY, eps_v, tol=tol, probe=probe)


def _measure(oracle, kind, op, scheme, which):
    """(ref, d_perm, d_newton, tol) and the conditions on the inputs, on the reference alone"""
    touching, ys = [], []
    eps = None if _scene(kind, which)[3] is None else _scene(kind, which)[3] * _modal(kind)["dt"]

    def probe(step, mp, u, v):
        touching.append(mp.in_contact(u))
        ys.extend(mp.slips(u, v, _modal(kind)["dt"]) if v is not None else mp.slips(u))

    tol_n = _newton_tol(kind, which, scheme)
    _reference_trajectory(oracle, kind, op, scheme, which, probe=probe, tol=tol_n)
    assert sum(touching) >= STEPS // 4, (kind, op, scheme, which, sum(touching))
    if which == "belt":
        assert min(ys) < eps <= max(ys), (kind, op, scheme, min(ys), max(ys), eps)
    return mr.measured_tolerance(lambda perm, tol: _reference_trajectory(oracle, kind, op, scheme, which, perm, tol), tol_n)


CENTRAL_CASES = [(k, o, "central", s) for k in KINDS for o in ("elastic", "neo_hookean") for s in ("ball", "belt")]
IMPLICIT_CASES = [(k, o, sc, s) for k, o in (("HEX8", "elastic"), ("TET4", "elastic"), ("HEX8", "neo_hookean")) for sc in ("euler", "newmark")
                  for s in ("ball", "belt")]
# measured on the CPU with the reference alone (_measure): d_perm, d_newton and the tolerance 20 (d_perm + d_newton), floored at 1e-13
TRAJECTORY_TOLERANCE = {
    ('HEX8', 'elastic', 'central', 'ball'): (1.5e-14, 0.0e+00, 3.1e-13),
    ('HEX8', 'elastic', 'central', 'belt'): (2.7e-14, 0.0e+00, 5.3e-13),
    ('HEX8', 'neo_hookean', 'central', 'ball'): (1.9e-14, 0.0e+00, 3.8e-13),
    ('HEX8', 'neo_hookean', 'central', 'belt'): (3.0e-14, 0.0e+00, 6.1e-13),
    ('TET4', 'elastic', 'central', 'ball'): (2.2e-14, 0.0e+00, 4.4e-13),
    ('TET4', 'elastic', 'central', 'belt'): (2.3e-14, 0.0e+00, 4.7e-13),
    ('TET4', 'neo_hookean', 'central', 'ball'): (1.3e-14, 0.0e+00, 2.7e-13),
    ('TET4', 'neo_hookean', 'central', 'belt'): (1.7e-14, 0.0e+00, 3.4e-13),
    ('QUAD4', 'elastic', 'central', 'ball'): (1.2e-14, 0.0e+00, 2.5e-13),
    ('QUAD4', 'elastic', 'central', 'belt'): (1.3e-14, 0.0e+00, 2.6e-13),
    ('QUAD4', 'neo_hookean', 'central', 'ball'): (1.1e-14, 0.0e+00, 2.1e-13),
    ('QUAD4', 'neo_hookean', 'central', 'belt'): (1.6e-14, 0.0e+00, 3.2e-13),
    ('TRI3', 'elastic', 'central', 'ball'): (7.7e-15, 0.0e+00, 1.5e-13),
    ('TRI3', 'elastic', 'central', 'belt'): (2.3e-14, 0.0e+00, 4.6e-13),
    ('TRI3', 'neo_hookean', 'central', 'ball'): (7.1e-15, 0.0e+00, 1.4e-13),
    ('TRI3', 'neo_hookean', 'central', 'belt'): (1.2e-14, 0.0e+00, 2.5e-13),
    ('HEX8_776', 'elastic', 'central', 'ball'): (1.0e-14, 0.0e+00, 2.1e-13),
    ('HEX8_776', 'elastic', 'central', 'belt'): (6.3e-15, 0.0e+00, 1.3e-13),
    ('HEX8_776', 'neo_hookean', 'central', 'ball'): (1.1e-14, 0.0e+00, 2.3e-13),
    ('HEX8_776', 'neo_hookean', 'central', 'belt'): (9.1e-15, 0.0e+00, 1.8e-13),
    ('HEX27', 'elastic', 'central', 'ball'): (1.1e-14, 0.0e+00, 2.1e-13),
    ('HEX27', 'elastic', 'central', 'belt'): (1.9e-14, 0.0e+00, 3.8e-13),
    ('HEX27', 'neo_hookean', 'central', 'ball'): (8.6e-15, 0.0e+00, 1.7e-13),
    ('HEX27', 'neo_hookean', 'central', 'belt'): (1.2e-14, 0.0e+00, 2.5e-13),
    ('HEX8', 'elastic', 'euler', 'ball'): (9.7e-14, 2.3e-11, 4.6e-10),
    ('HEX8', 'elastic', 'euler', 'belt'): (2.1e-13, 1.8e-11, 3.7e-10),
    ('HEX8', 'elastic', 'newmark', 'ball'): (1.0e-13, 9.7e-11, 1.9e-09),
    ('HEX8', 'elastic', 'newmark', 'belt'): (5.9e-14, 8.8e-11, 1.8e-09),
    ('TET4', 'elastic', 'euler', 'ball'): (3.1e-14, 2.1e-11, 4.2e-10),
    ('TET4', 'elastic', 'euler', 'belt'): (1.5e-13, 4.5e-11, 9.1e-10),
    ('TET4', 'elastic', 'newmark', 'ball'): (3.4e-14, 1.5e-11, 3.0e-10),
    ('TET4', 'elastic', 'newmark', 'belt'): (2.0e-14, 1.9e-11, 3.9e-10),
    ('HEX8', 'neo_hookean', 'euler', 'ball'): (9.8e-14, 1.2e-10, 2.4e-09),
    ('HEX8', 'neo_hookean', 'euler', 'belt'): (1.7e-13, 2.1e-11, 4.3e-10),
    ('HEX8', 'neo_hookean', 'newmark', 'ball'): (5.9e-14, 6.4e-11, 1.3e-09),
    ('HEX8', 'neo_hookean', 'newmark', 'belt'): (7.1e-14, 0.0e+00, 1.4e-12),
}


def _moving_integrator(engine, kind, op, scheme, which):
    """the integrator of a scene on a new assembler, its state set"""
    obs, paths, mu, eps_v = _scene(kind, which)
    dt = _modal(kind)["dt"]
    ti = _integrator(scheme, _assembler(engine, kind, op), kind, dt, newton_tol=_newton_tol(kind, which, scheme))
    ti.with_obstacles(_fa_obstacles(obs, mu, paths, slip_velocity=eps_v))
    n = _mesh(kind)[0].vertices.size
    ti.set_state(np.zeros(n), np.zeros(n))
    return ti


def _device_trajectory(engine, kind, op, scheme, which, cuts=(STEPS,)):
    ti = _moving_integrator(engine, kind, op, scheme, which)
    rows = []
    for count in cuts:
        rec = ti.step(count, record_every=EVERY if len(cuts) == 1 else 0)
        rows.append(_records(rec))
        assert rec.steps_done == count
    u, v, a, _, step = ti.state()
    assert step == sum(cuts)
    return (u, v, a, np.concatenate(rows)), ti, rec


TILED = "k_element_pass_tiled + k_dynamics_from_partials"
DAMPED_TILED = "k_damped_pass_tiled + k_dynamics_from_partials"
COMPOSED = "k_residual_elements + k_vector_from_elements_soa + k_dynamics_update"
COMPOSED_CONTACT = "k_residual_elements + k_vector_from_elements_soa + k_contact_force + k_dynamics_update"


def assert_step_route(engine, ti, kind, contact, damped=False):
    """ti: a central-difference integrator whose state has just been set, with its paths and motions.  ti.state() forms a_0 with the
    launch every step makes (read here because a record's energy pass replaces the name after a step): on the tiles it is the element
    pass and the fused node pass and nothing else -- no fall-back to the composed route, no launch added for the clock or the motion --
    and off them (HEX27) the composed route, with exactly one k_contact_force when there are obstacles"""
    ti.state()
    name = engine.last_kernel_name()
    if kind == "HEX27":
        want = COMPOSED_CONTACT if contact else COMPOSED
    else:
        want = DAMPED_TILED if damped else TILED
    assert name == want and name.count("k_contact_force") == (1 if contact and kind == "HEX27" else 0), (kind, name)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,op,scheme,which", CENTRAL_CASES + IMPLICIT_CASES)
def test_trajectory_with_moving_obstacles(engine, oracle, kind, op, scheme, which):
    """16 steps with a record every 4 under a pressed, held and retracted ball, or over a sliding frictional floor: u, v, a and the four
    record columns against the reference; and no launch is added per step: one residual per step (stats), and a central-difference launch
    is still the element pass and the fused node pass on the tiles, the composed route with one k_contact_force off them (last_kernel)"""
    ref, d_perm, d_newton, tol = _measure(oracle, kind, op, scheme, which)
    tol = mr.check_constants(TRAJECTORY_TOLERANCE, (kind, op, scheme, which), d_perm, d_newton, tol)
    got, ti, rec = _device_trajectory(engine, kind, op, scheme, which)
    mr.assert_parity(got, ref, tol, f"{kind} {op} {scheme} {which}")
    if scheme == "central":
        assert rec.stats[1] == STEPS + 1                           # a_0 and one residual per step: the clock adds no pass
    cur, lag = fa.Contact(engine).obstacle_offsets()               # the context is left at the clock of the last step
    obs, paths, _, _ = _scene(kind, which)
    dt = _modal(kind)["dt"]
    d = cur.shape[1]
    assert np.array_equal(cur[0], mr.path_offset(paths[0], STEPS * dt)[:d]) and np.array_equal(lag[0], mr.path_offset(paths[0], (STEPS - 1) * dt)[:d])
    if scheme == "central":
        ti.close()
        t2 = _moving_integrator(engine, kind, op, scheme, which)
        assert_step_route(engine, t2, kind, contact=True)
        t2.close()


# ------------------------------------------------------------------------------------------ GPU 8: off means off (the paths)
@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["central", "euler", "newmark"])
def test_paths_that_do_not_move_change_no_bit(scheme):
    """paths with no knots and paths with all-zero offsets give the bits of a run that never made the calls, with friction on"""
    kind = "HEX8"
    obs, _, mu, eps_v = _scene(kind, "belt")
    dt = _modal(kind)["dt"]
    n = _mesh(kind)[0].vertices.size
    v0 = 0.05 * np.random.default_rng(3).uniform(-1.0, 1.0, n)

    def run(paths):
        eng = fa.Engine(0)
        try:
            ti = _integrator(scheme, _assembler(eng, kind, "neo_hookean"), kind, dt, newton_tol=_newton_tol(kind, "belt", scheme))
            ti.with_obstacles(_fa_obstacles(obs, mu, None, slip_velocity=eps_v))
            if paths == "no knots":
                eng._check(eng._lib.fh_set_obstacle_paths(eng._h, _ffi.up(np.zeros(2, dtype=np.uint64)), None, None))
            elif paths == "zero offsets":
                ti.with_obstacles(_fa_obstacles(obs, mu, [([0.0, 4 * dt, 16 * dt], np.zeros((3, 3)))], slip_velocity=eps_v))
            ti.set_state(np.zeros(n), v0)
            rec = ti.step(6 if scheme != "central" else STEPS, record_every=EVERY)
            con = fa.Contact(eng)
            return list(ti.state()[:3]) + [_records(rec), con.force(), con.friction_force(), np.array([con.energy(), con.friction_potential()])]
        finally:
            eng.close()

    plain = run(None)
    assert np.abs(plain[4]).max() > 0.0 and np.abs(plain[5]).max() > 0.0      # contact and friction act
    for paths in ("no knots", "zero offsets"):
        for i, (p, q) in enumerate(zip(plain, run(paths))):
            assert np.array_equal(p, q), (paths, i)


# ------------------------------------------------------------------------------------------ GPU 7: cuts (the paths; both motions: test_boundary_motion.py)
@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["central", "euler", "newmark"])
def test_cut_runs_over_a_sliding_floor_repeat_bit_for_bit(scheme):
    """16 steps in one call against calls of 5 + 1 + 10 steps, and a second identical run: identical bits in u, v, a and the last record,
    as tests/test_dynamics.py holds every scheme to"""
    kind = "HEX8"

    def run(cuts):
        eng = fa.Engine(0)
        try:
            got, ti, _ = _device_trajectory(eng, kind, "neo_hookean", scheme, "belt", cuts)
            if scheme == "central":
                ti.close()
                t2 = _moving_integrator(eng, kind, "neo_hookean", scheme, "belt")
                assert_step_route(eng, t2, kind, contact=True)
                t2.close()
            return got[0], got[1], got[2], got[3][-1]
        finally:
            eng.close()

    base = run((STEPS,))
    assert np.abs(base[0]).max() > 0.0
    for cuts in ((STEPS,), (5, 1, 10)):
        for name, p, q in zip("uvar", base, run(cuts)):
            assert np.array_equal(p, q), (scheme, cuts, name)


# ------------------------------------------------------------------------------------------ GPU 10: arguments and scope
@pytest.mark.gpu
def test_arguments_and_scope(engine):
    kind = "HEX8"
    asm = _assembler(engine, kind, "elastic")
    lib, h = engine._lib, engine._h
    begin = lambda *b: _ffi.up(np.array(b, dtype=np.uint64))
    f64 = lambda *x: _ffi.fp(np.array(x, dtype=np.float64))
    code = lambda rc: rc
    # no obstacles: FH_INVALID_STATE
    assert code(lib.fh_set_obstacle_paths(h, begin(0, 1), f64(0.0), f64(0.0, 0.0, 0.0))) == FH_INVALID_STATE
    assert code(lib.fh_set_obstacle_time(h, 1.0, 0.0)) == FH_INVALID_STATE
    assert code(lib.fh_obstacle_offsets(h, f64(0, 0, 0), None)) == FH_INVALID_STATE
    obs = [("half_space", (0.0, 0.0, 0.3), (0.0, 0.0, 1.0), 1.0e3), ("ball", (0.5, 0.5, 1.5), 0.6, 1.0e3)]
    paths = [([0.0, 1.0], [[0.0, 0.0, 0.0], [0.5, 0.0, 0.0]]), None]
    engine.set_obstacles(_fa_obstacles(obs, None, paths))
    engine.set_obstacle_time(0.5, 0.25)
    con = fa.Contact(engine)
    before = con.obstacle_offsets()
    assert np.array_equal(before[0], [[0.25, 0.0, 0.0], [0.0, 0.0, 0.0]]) and np.array_equal(before[1], [[0.125, 0.0, 0.0], [0.0, 0.0, 0.0]])
    bad = [(begin(0, 2, 2), f64(0.0, 0.0), f64(*[0.0] * 6)),             # times not strictly increasing
           (begin(0, 2, 2), f64(1.0, 0.5), f64(*[0.0] * 6)),
           (begin(0, 2, 2), f64(0.0, np.inf), f64(*[0.0] * 6)),          # a non-finite time
           (begin(0, 2, 2), f64(0.0, 1.0), f64(0.0, np.nan, 0.0, 0.0, 0.0, 0.0)),   # a non-finite offset
           (begin(1, 2, 2), f64(0.0, 1.0), f64(*[0.0] * 6)),             # knot_begin does not start at 0
           (begin(0, 2, 1), f64(0.0, 1.0), f64(*[0.0] * 6))]             # knot_begin decreases
    for args in bad:
        assert code(lib.fh_set_obstacle_paths(h, *args)) == FH_BAD_ARGUMENT
        after = con.obstacle_offsets()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])      # the state is left as it was
    for t, t_lag in ((np.nan, 0.0), (0.0, np.inf)):
        assert code(lib.fh_set_obstacle_time(h, t, t_lag)) == FH_BAD_ARGUMENT
        assert np.array_equal(before[0], con.obstacle_offsets()[0])
    assert code(lib.fh_contact_resultants(h, None, None)) == FH_BAD_ARGUMENT
    # NULL arrays clear the paths; fh_set_obstacles clears them too and returns the clock to (0, 0)
    assert code(lib.fh_set_obstacle_paths(h, None, None, None)) == 0 and not con.obstacle_offsets()[0].any()
    engine.set_obstacles(_fa_obstacles(obs, None, paths))
    assert not con.obstacle_offsets()[0].any()                                   # the clock is back at (0, 0): d(0) = 0
    engine.set_obstacle_time(0.5)
    assert con.obstacle_offsets()[0][0, 0] == 0.25 and con.obstacle_offsets()[1][0, 0] == 0.25      # t_lag None: t
    engine.set_obstacles(_fa_obstacles(obs))
    engine.set_obstacle_time(0.5)
    assert not con.obstacle_offsets()[0].any()                                   # no paths any more
    # the count is the library's: obstacles set through the C interface, and cleared, are seen
    one = (_ffi.Obstacle * 1)()
    fa.Ball((0.5, 0.5, 1.5), 0.6, 1.0e3)._fill(one[0])
    assert code(lib.fh_set_obstacles(h, one, 1, None)) == 0 and con.obstacle_offsets()[0].shape == (1, 3) and con.resultants()[0].shape == (1, 3)
    assert code(lib.fh_set_obstacles(h, one, 0, None)) == 0 and con._count() == 0
    assert code(lib.fh_obstacle_count(h, None)) == FH_BAD_ARGUMENT
    # fh_dynamics_set_state returns the clock to (0, 0); a first-order handle refuses paths
    ti = fa.CentralDifference(asm, RHO, 1e-3).with_obstacles(_fa_obstacles(obs, None, paths))
    engine.set_obstacle_time(0.5, 0.25)
    ti.set_state(np.zeros(asm.engine.num_nodes() * 3))
    assert not con.obstacle_offsets()[0].any() and not con.obstacle_offsets()[1].any()
    ti.step(4)
    assert con.obstacle_offsets()[0][0, 0] == mr.path_offset(paths[0], 4 * 1e-3)[0] and con.obstacle_offsets()[1][0, 0] == mr.path_offset(paths[0], 3 * 1e-3)[0]
    ti.close()
    for fo in (fa.ForwardEuler(asm, RHO, 1e-4), fa.ThetaMethod(asm, RHO, 1e-2)):
        fo.with_obstacles(_fa_obstacles(obs, None, paths))
        fo.set_state(np.zeros(asm.engine.num_nodes() * 3))
        assert _code(fo.step, 1) == FH_UNSUPPORTED and "path" in engine.last_error()
        assert _code(fo.state) == FH_UNSUPPORTED
        fo.with_obstacles(_fa_obstacles(obs))
        assert _code(fo.step, 1) == 0                                             # ... and without paths it runs
        fo.close()
