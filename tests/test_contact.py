"""Penalty contact with rigid obstacles (fh_set_obstacles, fh_contact_*, fenris_amd.contact) against the NumPy statement of
tests/contact_reference.py, which is pinned here on the CPU against central differences of its own energy and force.

Bounds.  The term itself is a short sum per node: 1e-13 max|.| (the parity bound for short sums of test_independent_restatement.py).
Where the term rides on K(u) x, r(u) or a trajectory, the bound is measured from the reference alone, as test_dynamics.py measures its
own: d_perm, the reference against itself under another numbering, d_newton, the reference under a Newton tolerance 100 times smaller,
and the bound max(20 (d_perm + d_newton), 1e-13).  The constants measured on the CPU are recorded in MEASURED below; the tests measure
them again and print them."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import fenris_amd as fa
from fenris_amd import _ffi, quadrature

import contact_reference as cr
import dynamics_reference as dr

LAME = fa.LameParameters(384.0, 577.0)
RHO = 1.0
FH_BAD_ARGUMENT, FH_INVALID_STATE, FH_UNSUPPORTED = 2, 5, 6
OKIND = {"QUAD4": 0, "HEX8": 1, "TET4": 2, "HEX27": 3, "TRI3": 4, "TET10": 5}
NEW = ("fh_set_obstacles", "fh_contact_energy", "fh_contact_force_dev", "fh_contact_gap_dev", "fh_add_contact_tangent_csr_dev")
SHORT_SUM = 1e-13

# measured on the CPU with the reference alone: (d_perm, d_newton, bound = max(20 (d_perm + d_newton), 1e-13)); the tests measure them again
MEASURED = {"pressed HEX8 elastic": (1.7e-16, 1.0e-15, 1.0e-13), "pressed HEX8 neo_hookean": (2.2e-15, 0.0, 1.0e-13),
            "pressed HEX8 stable": (1.4e-20, 0.0, 1.0e-13), "pressed TET4 elastic": (4.2e-16, 1.9e-15, 1.0e-13),
            "pressed TET4 neo_hookean": (5.3e-16, 8.7e-16, 1.0e-13), "pressed TET4 stable": (5.4e-19, 0.0, 1.0e-13),
            "corner HEX8 elastic": (5.3e-16, 2.7e-15, 1.0e-13), "corner HEX8 neo_hookean": (2.0e-15, 0.0, 1.0e-13),
            "corner TET4 elastic": (1.8e-15, 4.5e-15, 1.3e-13), "corner TET4 neo_hookean": (2.7e-15, 4.7e-15, 1.5e-13),
            "indenter HEX8_6 neo_hookean": (9.1e-16, 1.2e-11, 2.4e-10),     # (Gauss-Newton: linear convergence, so the tolerance shows)
            "drop HEX8 neo_hookean, 64 steps": (1.9e-14, 0.0, 3.8e-13), "drop TET4 elastic, 64 steps": (3.0e-14, 0.0, 6.0e-13),
            "newmark, 4 steps": (4.2e-15, 0.0, 1.0e-13), "euler, 4 steps": (1.7e-14, 0.0, 3.3e-13), "RKL, 6 steps of 4 stages": (4.7e-16, 0.0, 1.0e-13),
            "shifted map, every route": (5e-16, 0.0, 1.0e-13)}


@pytest.fixture()
def engine():
    eng = fa.Engine(0)
    yield eng
    eng.close()


# ------------------------------------------------------------------------------------------ meshes, obstacles, problems
@functools.lru_cache(maxsize=None)
def _mesh(kind):
    P, T, Q = fa.procedural, quadrature.tensor, quadrature.total_order
    make = {"HEX8": (lambda: P.create_unit_box_uniform_hex_mesh_3d(2), T.hexahedron_gauss(2)),
            "HEX8_3": (lambda: P.create_unit_box_uniform_hex_mesh_3d(3), T.hexahedron_gauss(2)),
            "HEX8_6": (lambda: P.create_unit_box_uniform_hex_mesh_3d(6), T.hexahedron_gauss(2)),
            "HEX8_7": (lambda: P.create_unit_box_uniform_hex_mesh_3d(7), T.hexahedron_gauss(2)),   # 512 nodes, 343 elements: two of each
            "TET4": (lambda: P.create_unit_box_uniform_tet_mesh_3d(2), Q.tetrahedron(2)),
            "QUAD4": (lambda: P.create_unit_square_uniform_quad_mesh_2d(3), T.quadrilateral_gauss(2)),
            "TRI3": (lambda: P.create_unit_square_uniform_tri_mesh_2d(3), Q.triangle(2)),
            "TET10": (lambda: fa.tet10_mesh_from_tet4(P.create_unit_box_uniform_tet_mesh_3d(2)), Q.tetrahedron(4))}
    gen, (w, p) = make[kind]
    return gen(), np.asarray(w), np.asarray(p)


PARITY_KINDS = ["HEX8", "TET4", "QUAD4", "TRI3", "TET10", "HEX8_7"]


def _okind(kind):
    return OKIND[kind.split("_")[0]]


def _three_kinds(d):
    """the three kinds together on the unit square / cube: each reaches some nodes and leaves others"""
    if d == 3:
        return [("half_space", (0.3, 0.3, 0.3), (1.0, 2.0, 3.0), 1.0e4), ("ball", (1.1, 1.1, 1.1), 0.7, 2.0e3),
                ("cavity", (0.4, 0.5, 0.6), 0.75, 5.0e3)]
    return [("half_space", (0.3, 0.3), (1.0, 2.0), 1.0e4), ("ball", (1.1, 1.1), 0.7, 2.0e3), ("cavity", (0.4, 0.5), 0.6, 5.0e3)]


def _random_u(m, seed=1, size=0.02):
    return np.random.default_rng(seed).uniform(-size, size, m.vertices.size)


def _assert_precondition(obstacles, X, u):
    """every (node, obstacle) pair is clear of the switch phi = 0, and every obstacle has active and inactive nodes"""
    phi = cr.phi_table(obstacles, X, u)
    assert np.abs(phi).min() >= 1e-6, np.abs(phi).min()
    for row in phi:
        assert (row < 0).sum() >= 3 and (row > 0).sum() >= 3, ((row < 0).sum(), (row > 0).sum())


def _fa_obstacles(obstacles, node_weights=None):
    out = []
    for kind, p, q, k in obstacles:
        out.append(fa.HalfSpace(p, q, k) if kind == "half_space" else fa.Ball(p, q, k) if kind == "ball" else fa.Cavity(p, q, k))
    return fa.Obstacles(out, node_weights)


def _oop(oracle, op):
    return {"elastic": oracle.LINEAR_ELASTIC, "neo_hookean": oracle.NEO_HOOKEAN}[op]


def _material(op):
    return {"elastic": fa.LinearElasticMaterial, "neo_hookean": fa.NeoHookeanMaterial, "stable": fa.StableNeoHookeanMaterial}[op]()


def _lame(op, d=3):
    return LAME.for_stable_neo_hookean(d) if op == "stable" else LAME


class _StableProblem(cr.ContactMixin, dr.Problem):
    """the problem on the long-double reference of the Stable Neo-Hookean law (stable_neo_hookean_reference), rounded to double"""

    def __init__(self, kind, m, w, p, dirichlet=(), f=None, perm=None, obstacles=(), node_weights=None):
        import stable_neo_hookean_reference as snh

        self.snh = snh
        conn = np.asarray(m.connectivity)
        self.conn = conn if perm is None else conn[np.random.default_rng(perm).permutation(len(conn))]
        self.kind, self.vertices, self.w, self.p, self.lame, self.rho = kind.split("_")[0], np.asarray(m.vertices), w, p, _lame("stable"), RHO
        self.d = self.s = self.vertices.shape[1]
        self.N = len(self.vertices)
        self.n = self.s * self.N
        self.free = np.ones(self.n, dtype=bool)
        for k in range(self.s):
            self.free[self.s * np.asarray(dirichlet, dtype=np.int64) + k] = False
        self.f = np.zeros(self.n) if f is None else np.asarray(f, dtype=np.float64).reshape(-1)
        self.load_factor, self.direct, self._mass = None, "dense", None
        self.set_contact(obstacles, node_weights)

    def ref(self, u):
        return self.snh.Reference(self.kind, self.vertices, self.conn, self.w, self.p, u, self.lame.mu, self.lame.lambda_, rho=self.rho)

    def _base_residual(self, u):
        return self.ref(u).residual().astype(np.float64)

    def _base_energy(self, u):
        return float(self.ref(u).energy())

    def _base_tangent(self, u):
        ref = self.ref(u)
        ro, ci = ref.pattern()
        return sp.csr_matrix((ref.csr_values(ro, ci, "K").astype(np.float64), ci, ro), shape=(self.n, self.n))

    def mass(self):
        if self._mass is None:
            ref = self.ref(np.zeros(self.n))
            ro, ci = ref.pattern()
            self._mass = sp.csr_matrix((ref.csr_values(ro, ci, "M").astype(np.float64), ci, ro), shape=(self.n, self.n))
        return self._mass


def _problem(oracle, kind, op, obstacles=(), dirichlet=(), f=None, perm=None, node_weights=None, rho=RHO, groups=None):
    """the reference's problem; perm: a permutation of the connectivity rows (another summation order in r, nothing else)"""
    m, w, p = _mesh(kind)
    if op == "stable":
        return _StableProblem(kind, m, w, p, dirichlet, f, perm, obstacles, node_weights)
    if groups is None:
        groups = [(np.asarray(m.connectivity), w, p)]
    if perm is not None:
        groups = [(c[np.random.default_rng(perm + g).permutation(len(c))], wg, pg) for g, (c, wg, pg) in enumerate(groups)]
    return cr.ContactProblem(oracle, _okind(kind), _oop(oracle, op), m.vertices, groups, params=LAME.as_pair(), rho=rho, dirichlet=dirichlet, f=f,
                             obstacles=obstacles, node_weights=node_weights)


def _assembler(engine, kind, op, u=None, qt=None):
    m, w, p = _mesh(kind)
    d = m.vertices.shape[1]
    if qt is None:
        qt = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(_lame(op, d))
    return (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(m).with_operator(fa.MaterialEllipticOperator(_material(op)))
            .with_quadrature_table(qt).with_u(np.zeros(m.vertices.size) if u is None else u).build())


def _rel(x, y):
    return np.abs(np.asarray(x) - np.asarray(y)).max() / max(np.abs(np.asarray(y)).max(), 1e-300)


def _check(name, err, tol):
    print(f"{name}: {err:.3e} (bound {tol:.3e})")
    assert err <= tol, (name, err, tol)


def _face(m, axis, value):
    return np.where(np.isclose(m.vertices[:, axis], value))[0]


# ------------------------------------------------------------------------------------------ no GPU: declarations, the reference pinned
def test_contact_entry_points_are_declared():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fenris_hip.h")).read()
    for name in NEW:
        assert name in _ffi.exported_symbols() and name + "(" in hdr
    for text in ("FH_OBSTACLE_HALF_SPACE = 0, FH_OBSTACLE_BALL = 1, FH_OBSTACLE_CAVITY = 2", "#define FH_MAX_OBSTACLES 16", "} fh_obstacle;",
                 "#define FH_ABI_VERSION 1"):
        assert text in hdr
    for cls in (fa.MatrixFreeTangent, fa.MatrixFreeShiftedTangent, fa.MatrixFreeNewton, fa.TimeIntegrator, fa.MatrixFreeEigensolver):
        assert callable(getattr(cls, "with_obstacles"))
    assert not hasattr(fa.MatrixFreeOperator, "with_obstacles")   # the operator's own map leaves the term out
    assert callable(fa.Engine.set_obstacles) and (fa.contact.OBSTACLE_HALF_SPACE, fa.contact.OBSTACLE_BALL, fa.contact.OBSTACLE_CAVITY) == (0, 1, 2)
    o = _ffi.Obstacle()
    fa.Cavity((1.0, 2.0), 0.5, 3.0)._fill(o)
    assert (o.kind, o.stiffness, o.radius, list(o.point), list(o.normal)) == (2, 3.0, 0.5, [1.0, 2.0, 0.0], [0.0, 0.0, 0.0])


@pytest.mark.parametrize("kind", ["HEX8", "QUAD4", "HEX8_3"])
def test_reference_force_is_the_derivative_of_the_energy(kind):
    """g against central differences of E_c, the three kinds together, random u of size 0.02"""
    m = _mesh(kind)[0]
    obs = _three_kinds(m.vertices.shape[1])
    u = _random_u(m)
    _assert_precondition(obs, m.vertices, u)
    g = cr.force(obs, m.vertices, u)
    h = 1e-6
    fd = np.zeros_like(g)
    for i in range(len(u)):
        e = np.zeros_like(u)
        e[i] = h
        fd[i] = (cr.energy(obs, m.vertices, u + e) - cr.energy(obs, m.vertices, u - e)) / (2 * h)
    _check(f"{kind} g vs dE_c", _rel(fd, g), 2e-9)


@pytest.mark.parametrize("kind", ["HEX8", "QUAD4", "HEX8_3"])
def test_reference_exact_tangent_is_the_derivative_of_the_force(kind):
    """B with the curvature kept against central differences of g; and the applied B is the exact one minus the ball's curvature"""
    m = _mesh(kind)[0]
    d = m.vertices.shape[1]
    obs = _three_kinds(d)
    u = _random_u(m)
    _assert_precondition(obs, m.vertices, u)
    B = cr.tangent(obs, m.vertices, u, exact=True).toarray()
    h = 1e-6
    fd = np.zeros_like(B)
    for i in range(len(u)):
        e = np.zeros_like(u)
        e[i] = h
        fd[:, i] = (cr.force(obs, m.vertices, u + e) - cr.force(obs, m.vertices, u - e)) / (2 * h)
    _check(f"{kind} B vs dg", _rel(fd, B), 2e-9)
    ball = [o for o in obs if o[0] == "ball"]
    dropped = cr.blocks(ball, m.vertices, u, exact=True) - cr.blocks(ball, m.vertices, u, exact=False)
    x = cr.positions(m.vertices, u)
    for i, xi in enumerate(x):
        phi, n, H = cr.phi_grad_hess(ball[0], xi)
        want = ball[0][3] * phi * H if phi < 0 else np.zeros((d, d))
        assert np.abs(dropped[i] - want).max() <= 1e-12 * ball[0][3]
    applied, exact = cr.blocks(obs, m.vertices, u, exact=False), cr.blocks(obs, m.vertices, u, exact=True)
    assert np.abs((exact - applied) - dropped).max() <= 1e-12 * 1e4   # half-space and cavity: exact


@pytest.mark.parametrize("kind", ["HEX8", "QUAD4"])
def test_reference_applied_tangent_is_positive_semidefinite(kind):
    m = _mesh(kind)[0]
    d = m.vertices.shape[1]
    u = _random_u(m, seed=3)
    for ob in _three_kinds(d):
        for exact in ((False, True) if ob[0] != "ball" else (False,)):
            B = cr.blocks([ob], m.vertices, u, exact=exact)
            assert np.abs(B - B.transpose(0, 2, 1)).max() == 0.0 or np.abs(B - B.transpose(0, 2, 1)).max() <= 1e-12 * ob[3]
            assert min(np.linalg.eigvalsh(b).min() for b in B) >= -1e-12 * ob[3], ob[0]
    ball = [o for o in _three_kinds(d) if o[0] == "ball"]
    assert min(np.linalg.eigvalsh(b).min() for b in cr.blocks(ball, m.vertices, u, exact=True)) < 0.0   # (why the curvature is dropped)


def test_reference_centre_node_and_strict_switch():
    """a node at the centre of a ball: energy, no force, no block; a node on the plane: inactive"""
    X = np.array([[0.5, 0.5, 0.5], [0.0, 0.0, 0.0], [0.0, 0.0, 0.5]])
    u = np.zeros(9)
    ball = [("ball", (0.5, 0.5, 0.5), 0.25, 100.0)]
    assert cr.energy(ball, X, u) == 0.5 * 100.0 * 0.25 ** 2 and not cr.force(ball, X, u).any() and not cr.blocks(ball, X, u).any()
    floor = [("half_space", (0.0, 0.0, 0.5), (0.0, 0.0, 1.0), 100.0)]
    assert cr.gap(floor, X, u).tolist() == [0.0, -0.5, 0.0]
    g = cr.force(floor, X, u).reshape(3, 3)
    assert not g[0].any() and not g[2].any() and g[1].tolist() == [0.0, 0.0, -50.0]


# ------------------------------------------------------------------------------------------ GPU: argument errors
def _code(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except fa.FenrisError as e:
        return e.code
    return 0


@pytest.mark.gpu
def test_set_obstacles_argument_errors(engine):
    floor = fa.HalfSpace((0, 0, 0), (0, 0, 1), 1e3)
    assert _code(engine.set_obstacles, [floor]) == FH_INVALID_STATE        # no mesh
    assert _code(engine.set_obstacles, None) == 0                         # clearing needs none
    asm = _assembler(engine, "HEX8", "elastic")
    N = asm.engine.num_nodes()
    assert _code(engine.set_obstacles, [floor] * 16) == 0
    bad = [[floor] * 17, [fa.HalfSpace((0, 0, 0), (0, 0, 0), 1e3)], [fa.HalfSpace((0, 0, 0), (0, 0, 1), 0.0)], [fa.HalfSpace((0, 0, 0), (0, 0, 1), -1.0)],
           [fa.Ball((0, 0, 0), 0.0, 1e3)], [fa.Cavity((0, 0, 0), -1.0, 1e3)], [fa.Ball((np.nan, 0, 0), 1.0, 1e3)], [fa.Ball((0, 0, 0), np.inf, 1e3)],
           [fa.HalfSpace((0, 0, 0), (0, np.inf, 1), 1e3)], [fa.HalfSpace((0, 0, 0), (0, 0, 1), np.nan)]]
    for obs in bad:
        assert _code(engine.set_obstacles, obs) == FH_BAD_ARGUMENT, obs
    unknown = fa.Ball((0, 0, 0), 1.0, 1e3)
    unknown.kind = 7
    assert _code(engine.set_obstacles, [unknown]) == FH_BAD_ARGUMENT
    w = np.ones(N)
    w[3] = -0.5
    assert _code(engine.set_obstacles, fa.Obstacles([floor], w)) == FH_BAD_ARGUMENT
    w[3] = 0.0
    assert _code(engine.set_obstacles, fa.Obstacles([floor], w)) == 0
    # a failed call leaves the obstacles as they were: one floor with weights
    assert _code(engine.set_obstacles, [floor] * 17) == FH_BAD_ARGUMENT
    asm.with_u(np.full(3 * N, -0.1))
    assert fa.Contact(engine).energy() > 0.0
    engine.set_obstacles(None)
    assert fa.Contact(engine).energy() == 0.0
    assert np.isinf(fa.Contact(engine).gap()).all()
    # without a pattern
    engine.set_obstacles([floor])
    import torch
    eng2 = fa.Engine(0)
    try:
        asm2 = _assembler(eng2, "HEX8", "elastic")
        eng2.set_obstacles([floor])
        assert _code(fa.Contact(eng2).add_tangent_to, torch.zeros(10, dtype=torch.float64, device="cuda:0")) == FH_INVALID_STATE
        assert asm2 is not None
    finally:
        eng2.close()


@pytest.mark.gpu
def test_laplace_and_multigrid_are_refused(engine):
    import torch

    m, w, p = _mesh("HEX8")
    qt = fa.UniformQuadratureTable.from_points_and_weights(p, w)
    asm = (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(m).with_operator(fa.LaplaceOperator()).with_quadrature_table(qt)
           .with_u(np.zeros(m.num_nodes())).build())
    floor = fa.Obstacles([fa.HalfSpace((0, 0, 0.1), (0, 0, 1), 1e3)])
    x = torch.ones(m.num_nodes(), dtype=torch.float64, device="cuda:0")
    t = fa.MatrixFreeTangent(asm).with_obstacles(floor)
    assert _code(t.apply, torch.empty_like(x), x) == FH_UNSUPPORTED
    assert _code(t.diagonal) == FH_UNSUPPORTED
    assert _code(t.cg_solve, x, torch.zeros_like(x)) == FH_UNSUPPORTED
    assert _code(fa.MatrixFreeNewton(asm).with_obstacles(floor).solve, np.zeros(m.num_nodes())) == FH_UNSUPPORTED
    assert _code(fa.MatrixFreeShiftedTangent(asm, 1.0, 1.0, 1.0).with_obstacles(floor).apply, torch.empty_like(x), x) == FH_UNSUPPORTED
    assert _code(lambda: fa.CentralDifference(asm, 1.0, 1e-3).with_obstacles(floor).step(1)) == FH_UNSUPPORTED
    assert _code(fa.MatrixFreeEigensolver(asm, 1.0).with_obstacles(floor).solve, 2) == FH_UNSUPPORTED
    fa.MatrixFreeOperator(asm).apply(torch.empty_like(x), x)            # the operator's own map: as before
    engine.set_obstacles(None)
    t.with_obstacles(None).apply(torch.empty_like(x), x)


@pytest.mark.gpu
def test_multigrid_with_obstacles_is_unsupported():
    coarse, w, p = _mesh("HEX8")
    eng = fa.Engine(0)
    try:
        m, transfer = fa.refine_uniformly_with_transfer(coarse)
        qt = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(LAME)
        asm = (fa.ElementEllipticAssemblerBuilder(eng).with_finite_element_space(m).with_operator(fa.MaterialEllipticOperator(fa.NeoHookeanMaterial()))
               .with_quadrature_table(qt).with_u(np.zeros(m.vertices.size)).build())
        mg = fa.GeometricMultigrid(asm, [coarse], [transfer])
        top = _face(m, 2, 1.0)
        floor = fa.Obstacles([fa.HalfSpace((0, 0, 0.02), (0, 0, 1), 1e4)])
        f = np.zeros(m.vertices.size)
        solver = fa.MatrixFreeNewton(asm).with_dirichlet_nodes(top).with_load(f).with_multigrid(mg).with_obstacles(floor)
        with pytest.raises(fa.FenrisError) as e:
            solver.solve(np.zeros_like(f), fa.NewtonSettings(10, 1e-8))
        assert e.value.code == FH_UNSUPPORTED and "MULTIGRID" in str(e.value)
        t = fa.MatrixFreeTangent(asm).with_dirichlet_nodes(top).with_multigrid(mg).with_obstacles(floor)
        assert _code(t.cg_solve, np.ones_like(f), np.zeros_like(f)) == FH_UNSUPPORTED
        t.with_obstacles(None)
        assert t.cg_solve(np.ones_like(f) * (1 - np.isin(np.arange(len(f)) // 3, top)), np.zeros_like(f), rel_tol=1e-6) > 0   # cleared: multigrid again
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------ GPU 1: the term itself
def _csr_of_contact(engine, asm):
    k = fa.CsrAssembler(fa.SCATTER_GATHER).assemble(asm)
    vals = np.zeros_like(k.values)
    fa.Contact(engine).add_tangent_to(vals)
    again = np.array(vals)
    fa.Contact(engine).add_tangent_to(again)       # ADDS
    assert np.array_equal(again, 2.0 * vals)
    return fa.CsrMatrix(k.row_offsets, k.col_indices, vals).to_scipy().toarray()


def _term_parity(engine, kind, op, obs, u, weights=None, tag=""):
    import torch

    m = _mesh(kind)[0]
    d = m.vertices.shape[1]
    X = m.vertices
    asm = _assembler(engine, kind, op, u)
    engine.set_obstacles(_fa_obstacles(obs, weights))
    con = fa.Contact(engine)
    e_ref, g_ref, gap_ref = cr.energy(obs, X, u, weights), cr.force(obs, X, u, weights), cr.gap(obs, X, u)
    B_ref = cr.tangent(obs, X, u, weights, exact=False).toarray()
    _check(f"{tag}{kind} energy", abs(con.energy() - e_ref) / max(abs(e_ref), 1e-300), SHORT_SUM)
    assert engine.last_kernel_name() == "k_contact_energy"
    _check(f"{tag}{kind} gap", _rel(con.gap(), gap_ref), SHORT_SUM)
    # the force ADDS into an array of garbage; what lies outside stays
    n = X.size
    garbage = np.random.default_rng(5).uniform(-1.0, 1.0, n + 64)
    buf = torch.tensor(garbage, device="cuda:0")
    con.force(device=True, out=buf[32:32 + n])
    got = buf.cpu().numpy()
    assert np.array_equal(got[:32], garbage[:32]) and np.array_equal(got[32 + n:], garbage[32 + n:])
    _check(f"{tag}{kind} force", np.abs(got[32:32 + n] - garbage[32:32 + n] - g_ref).max() / max(np.abs(g_ref).max(), 1.0), SHORT_SUM + 2.3e-16)
    _check(f"{tag}{kind} force alone", _rel(con.force(), g_ref), SHORT_SUM)
    _check(f"{tag}{kind} csr blocks", np.abs(_csr_of_contact(engine, asm) - B_ref).max() / max(np.abs(B_ref).max(), 1e-300), SHORT_SUM)
    # the tangent's map with the obstacles minus the same map without them
    x = np.random.default_rng(6).uniform(-1.0, 1.0, n)
    t = fa.MatrixFreeTangent(asm).with_obstacles(_fa_obstacles(obs, weights))
    y1 = t.apply(np.zeros(n), x).copy()
    name = engine.last_kernel_name()
    d1 = t.diagonal()
    assert engine.last_kernel_name() == "k_contact_diagonal"
    t.with_obstacles(None)
    y0, d0 = t.apply(np.zeros(n), x).copy(), t.diagonal()
    scale = max(np.abs(B_ref @ x).max(), 1e-300)
    _check(f"{tag}{kind} apply difference", np.abs((y1 - y0) - B_ref @ x).max() / max(scale, np.abs(y0).max()), SHORT_SUM)
    _check(f"{tag}{kind} diagonal difference", np.abs((d1 - d0) - B_ref.diagonal()).max() / max(np.abs(d1).max(), 1e-300), SHORT_SUM)
    return name


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["elastic", "neo_hookean"])
@pytest.mark.parametrize("kind", PARITY_KINDS)
def test_term_parity(engine, kind, op):
    """energy, force, gap, CSR blocks and the tangent's map with minus without obstacles, against the reference on the precondition inputs;
    every route: the tiles (one and two node workgroups) and off them"""
    m = _mesh(kind)[0]
    obs = _three_kinds(m.vertices.shape[1])
    u = _random_u(m)
    _assert_precondition(obs, m.vertices, u)
    name = _term_parity(engine, kind, op, obs, u)
    print(kind, op, name)
    if kind == "TET10":
        assert name.endswith("+ k_contact_apply"), name
    else:
        assert name.endswith("k_operator_from_partials"), name


@pytest.mark.gpu
def test_term_special_nodes(engine):
    """a ball centred on a node (energy, no force, no block); a plane through nodes with exactly representable coordinates at u = 0 (inactive);
    node weights with zeros"""
    kind = "HEX8"
    m = _mesh(kind)[0]
    X = m.vertices
    u = _random_u(m)
    centre = int(np.where(np.all(np.isclose(X, 0.5), axis=1))[0][0])
    u.reshape(-1, 3)[centre] = 0.0
    obs = [("ball", tuple(X[centre]), 0.3, 3e3)]
    assert cr.phi_table(obs, X, u)[0, centre] == -0.3
    _term_parity(engine, kind, "neo_hookean", obs, u, tag="centre ")
    engine.set_obstacles(_fa_obstacles(obs))
    assert fa.Contact(engine).force().reshape(-1, 3)[centre].tolist() == [0.0, 0.0, 0.0]
    # the plane z = 0.5 at u = 0: the mid nodes are on it, the bottom nodes below
    z = np.zeros(X.size)
    floor = [("half_space", (0.0, 0.0, 0.5), (0.0, 0.0, 2.0), 1e4)]
    _term_parity(engine, kind, "elastic", floor, z, tag="plane ")
    engine.set_obstacles(_fa_obstacles(floor))
    con = fa.Contact(engine)
    mid, bottom = _face(m, 2, 0.5), _face(m, 2, 0.0)
    gap, g = con.gap(), con.force().reshape(-1, 3)
    assert (gap[mid] == 0.0).all() and not g[mid].any() and (gap[bottom] == -0.5).all() and (g[bottom, 2] == -5e3).all()
    # weights with zeros
    w = np.random.default_rng(8).uniform(0.5, 2.0, len(X))
    w[::3] = 0.0
    obs3 = _three_kinds(3)
    _term_parity(engine, kind, "neo_hookean", obs3, _random_u(m), weights=w, tag="weights ")
    engine.set_obstacles(_fa_obstacles(obs3, w))
    assert not fa.Contact(engine).force().reshape(-1, 3)[::3].any()


# ------------------------------------------------------------------------------------------ GPU 2: every operator route
def _renumbered(prob_of, X, conn_groups, P):
    """the same problem with node j of the new numbering = node P[j] of the old"""
    inv = np.empty_like(P)
    inv[P] = np.arange(len(P))
    return prob_of(X[P], [(inv[np.asarray(c, dtype=np.int64)].astype(np.uint64), w, p) for c, w, p in conn_groups]), inv


def _shifted_reference(oracle, kind, op, groups, obs, u, x, alpha, beta, bc, P=None):
    """(alpha M + beta (K + B)) x and its diagonal with the Dirichlet rows scale x (scale: the first nonzero diagonal entry, in row order);
    P: evaluated on a renumbered mesh and mapped back"""
    m = _mesh(kind)[0]
    d = m.vertices.shape[1]
    X = np.asarray(m.vertices)

    def prob_of(Xn, gr):
        return cr.ContactProblem(oracle, _okind(kind), _oop(oracle, op), Xn, gr, params=LAME.as_pair(), rho=RHO, obstacles=obs)

    def dofs(nodes):
        return (d * np.asarray(nodes, dtype=np.int64)[:, None] + np.arange(d)).reshape(-1)

    if P is None:
        prob, un, xn, bcn = prob_of(X, groups), u, x, np.asarray(bc, dtype=np.int64)
    else:
        prob, inv = _renumbered(prob_of, X, groups, P)
        un, xn, bcn = u[dofs(P)], x[dofs(P)], inv[np.asarray(bc, dtype=np.int64)]
    A = (alpha * prob.mass() + beta * prob.tangent(un)).tocsr()
    diag = A.diagonal()
    fixed = np.zeros(prob.n, dtype=bool)
    if len(bcn):
        fixed[dofs(bcn)] = True
    xm = np.where(fixed, 0.0, xn)
    y = np.asarray(A @ xm).reshape(-1)
    if P is None:
        nz = np.nonzero(diag)[0]
        scale = abs(diag[nz[0]]) if len(nz) else 1.0
    else:   # (the scale is that of the original numbering's first row)
        scale = abs(diag[inv[0] * d]) if diag[inv[0] * d] != 0.0 else None
        assert scale is not None
    y = np.where(fixed, scale * xn, y)
    diag = np.where(fixed, scale, diag)
    if P is not None:
        back = dofs(inv)
        y, diag = y[back], diag[back]
    return y, diag


def _rule_set(kind):
    """two rules with different point sets over the elements of `kind` (Hex8): the table and the reference's groups"""
    m, w, p = _mesh(kind)
    w2, p2 = (np.asarray(a) for a in quadrature.tensor.hexahedron_gauss(3))
    emap = (np.arange(m.num_elements()) % 3 == 0).astype(np.uint64)
    qt = fa.compact_quadrature_table([p, p2], [w, w2], [[LAME] * len(w), [LAME] * len(w2)], emap)
    conn = np.asarray(m.connectivity)
    return qt, [(conn[emap == 0], w, p), (conn[emap == 1], w2, p2)]


ROUTES = [("HEX8", "neo_hookean", "uniform", "k_shifted_tangent_tiled + k_operator_from_partials"),       # shift_hex8_fused
          ("HEX8", "elastic", "uniform", "k_shifted_pass_tiled + k_operator_from_partials"),               # ... with the scaled operand
          ("HEX8_7", "neo_hookean", "uniform", "k_shifted_tangent_tiled + k_operator_from_partials"),     # two node workgroups
          ("TET4", "neo_hookean", "uniform", "k_tangent_tiled + k_operator_from_partials"),                # the tiles: tangent, then the shift node pass
          ("QUAD4", "elastic", "uniform", "k_element_pass_tiled + k_operator_from_partials"),
          ("TRI3", "neo_hookean", "uniform", "k_tangent_tiled + k_operator_from_partials"),
          ("TET10", "neo_hookean", "uniform", "k_mf_apply_elements + k_vector_from_elements_soa + k_contact_apply"),   # off the tiles
          ("TET10", "elastic", "uniform", "k_mf_apply_elements + k_vector_from_elements_soa + k_contact_apply"),
          ("HEX8", "neo_hookean", "rule_set", None)]


@pytest.mark.gpu
@pytest.mark.parametrize("dirichlet", [False, True])
@pytest.mark.parametrize("kind,op,table,kernel", ROUTES)
def test_shifted_map_on_every_route(engine, oracle, kind, op, table, kernel, dirichlet):
    """(M + beta (K + B)) x and its diagonal against the reference; with Dirichlet nodes the rows are scale x, scale from the diagonal with B"""
    m, w, p = _mesh(kind)
    d = m.vertices.shape[1]
    obs = _three_kinds(d)
    u = _random_u(m)
    _assert_precondition(obs, m.vertices, u)
    qt, groups = (None, [(np.asarray(m.connectivity), w, p)]) if table == "uniform" else _rule_set(kind)
    alpha, beta = 1.0, 0.37
    bc = _face(m, 0, 0.0) if dirichlet else np.zeros(0, dtype=np.int64)
    x = np.random.default_rng(9).uniform(-1.0, 1.0, m.vertices.size)
    y_ref, d_ref = _shifted_reference(oracle, kind, op, groups, obs, u, x, alpha, beta, bc)
    P = np.random.default_rng(10).permutation(len(m.vertices))
    P[np.where(P == 0)[0][0]], P[0] = P[0], 0      # (node 0 stays first: the scale of the Dirichlet rows is the first row's)
    y_perm, d_perm_ = _shifted_reference(oracle, kind, op, groups, obs, u, x, alpha, beta, bc, P)
    d_perm = max(_rel(y_perm, y_ref), _rel(d_perm_, d_ref))
    tol = max(20.0 * d_perm, 1e-13)
    asm = _assembler(engine, kind, op, u, qt)
    t = fa.MatrixFreeShiftedTangent(asm, RHO, alpha, beta).with_dirichlet_nodes(bc if dirichlet else None).with_obstacles(_fa_obstacles(obs))
    y = t.apply(np.zeros_like(x), x)
    name = engine.last_kernel_name()
    print(f"{kind} {op} {table} dirichlet={dirichlet}: {name}; d_perm {d_perm:.2e}")
    if kernel is not None:
        assert name == kernel, name
    _check("apply", _rel(y, y_ref), tol)
    _check("diagonal", _rel(t.diagonal(), d_ref), tol)
    # without the obstacles the map differs (the term is in it), and the plain tangent agrees with alpha = 0, beta = 1
    y0 = fa.MatrixFreeShiftedTangent(asm, RHO, alpha, beta).with_dirichlet_nodes(bc if dirichlet else None).with_obstacles(None).apply(np.zeros_like(x), x)
    assert _rel(y0, y_ref) > 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["HEX8", "TET10"])
def test_operator_entry_points_leave_the_term_out(engine, kind):
    """fh_apply_operator_dev, fh_operator_diagonal_dev and fh_cg_solve_matrix_free on linear elasticity: the same bits with and without obstacles"""
    m = _mesh(kind)[0]
    asm = _assembler(engine, kind, "elastic", _random_u(m))
    bc = _face(m, 0, 0.0)
    x = np.random.default_rng(11).uniform(-1.0, 1.0, m.vertices.size)
    b = np.where(np.isin(np.arange(len(x)) // 3, bc), 0.0, x)
    a = fa.MatrixFreeOperator(asm).with_dirichlet_nodes(bc)

    def run():
        sol = np.zeros_like(x)
        it = a.cg_solve(b, sol, rel_tol=1e-10)
        return a.apply(np.zeros_like(x), x).copy(), a.diagonal(), sol, it

    before = run()
    engine.set_obstacles(_fa_obstacles(_three_kinds(3)))
    after = run()
    for p, q in zip(before, after):
        assert np.array_equal(p, q)
    t = fa.MatrixFreeTangent(asm).with_dirichlet_nodes(bc)    # (owns no obstacles: the engine's stay) -- the tangent has the term
    assert not np.array_equal(t.apply(np.zeros_like(x), x), before[0])


# ------------------------------------------------------------------------------------------ GPU 3: no obstacles, no change
@pytest.mark.gpu
@pytest.mark.parametrize("kind,op", [("HEX8_3", "neo_hookean"), ("TET4", "elastic"), ("TET10", "neo_hookean")])
def test_no_obstacles_no_change(kind, op):
    """setting then clearing obstacles gives the bits of never setting them; obstacles no node reaches give equal values: the tangent's map,
    a Newton solve and 8 explicit steps"""
    m = _mesh(kind)[0]
    n = m.vertices.size
    top, bottom = _face(m, 2, 1.0), _face(m, 2, 0.0)
    x = np.random.default_rng(12).uniform(-1.0, 1.0, n)
    f = np.zeros(n)
    f[3 * top + 2] = -2.0
    far = fa.Obstacles([fa.HalfSpace((0, 0, -5.0), (0, 0, 1), 1e4), fa.Ball((9.0, 9.0, 9.0), 1.0, 1e4), fa.Cavity((0.5, 0.5, 0.5), 30.0, 1e4)])

    def run(mode):
        eng = fa.Engine(0)
        try:
            asm = _assembler(eng, kind, op, _random_u(m))
            if mode == "set_then_clear":
                eng.set_obstacles(_fa_obstacles(_three_kinds(3)))
                fa.MatrixFreeTangent(asm).with_dirichlet_nodes(bottom).apply(np.zeros(n), x)
                eng.set_obstacles(None)
            elif mode == "far":
                eng.set_obstacles(far)
            t = fa.MatrixFreeTangent(asm).with_dirichlet_nodes(bottom)
            y, dg = t.apply(np.zeros(n), x).copy(), t.diagonal()
            u = np.zeros(n)
            res = fa.MatrixFreeNewton(asm).with_dirichlet_nodes(bottom).with_load(f).solve(u, fa.NewtonSettings(30, 1e-9), linear_rel_tol=1e-10)
            if kind == "TET10":   # (no positive row-sum lumping for the explicit scheme on Tet10: 2 backward-Euler steps instead)
                ti = fa.BackwardEuler(asm, RHO, 1e-2).with_newton(fa.NewtonSettings(30, 1e-9), linear_rel_tol=1e-10)
                ti.with_dirichlet_nodes(bottom).with_load(f)
            else:
                ti = fa.CentralDifference(asm, RHO, 1e-3).with_dirichlet_nodes(bottom).with_load(f)
            ti.set_state(np.zeros(n), 0.01 * x)
            rec = ti.step(2 if kind == "TET10" else 8, 4)
            uu, vv, aa, _, _ = ti.state()
            ti.close()
            return y, dg, u, np.array([res.iterations, res.linear_iterations, res.residual_norm]), uu, vv, aa, rec.kinetic, rec.stored
        finally:
            eng.close()

    never = run("never")
    for mode in ("set_then_clear", "far"):
        got = run(mode)
        for i, (p, q) in enumerate(zip(never, got)):
            assert np.array_equal(p, q), (mode, i)


# ------------------------------------------------------------------------------------------ GPU 4: Newton
# |F| <= 1e-11: small enough that the device, whose Newton steps come from a PCG to 1e-13 (an error of cond x 1e-13 in the step), takes the
# iteration that removes that error, as the reference's direct solves need not; the rounding floor of |F| in these scenes is some 1e-13
NEWTON_TOLERANCE = 1e-11
def _newton_tolerances(oracle, kind, op, obs, bc, f, u0, tol):
    """reference Newton with direct solves: (u, d_perm, d_newton, bound, iterations)"""
    def solve(perm, t):
        prob = _problem(oracle, kind, op, obs, bc, f, perm)

        def F(x):
            out = prob.residual(x) - prob.f
            out[~prob.free] = 0.0
            return out

        st, u, it = dr.newton(prob, F, prob.tangent, u0.copy(), t)
        assert st == "ok", st
        return u, it, prob

    u, it, prob = solve(None, tol)
    d_perm = _rel(solve(7, tol)[0], u)
    d_newton = _rel(solve(None, tol / 100.0)[0], u)
    return u, d_perm, d_newton, max(20.0 * (d_perm + d_newton), 1e-13), it, prob


def _device_newton(engine, kind, op, obs, bc, f, u0, tol):
    asm = _assembler(engine, kind, op)
    solver = fa.MatrixFreeNewton(asm).with_dirichlet_nodes(bc if len(bc) else None).with_load(f).with_obstacles(_fa_obstacles(obs))
    u = u0.copy()
    res = solver.solve(u, fa.NewtonSettings(40, tol), line_search=fa.BacktrackingLineSearch(), preconditioner=_ffi.PRECOND_JACOBI, linear_rel_tol=1e-13)
    return u, res


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["elastic", "neo_hookean", "stable"])
@pytest.mark.parametrize("kind", ["HEX8", "TET4"])
def test_newton_pressed_block(engine, oracle, kind, op):
    """(a) the cube's top face held at u_z = -0.05 over the floor z >= 0.02, k = 1e4: the bottom nodes end up in the floor"""
    m = _mesh(kind)[0]
    n = m.vertices.size
    obs = [("half_space", (0.0, 0.0, 0.02), (0.0, 0.0, 1.0), 1.0e4)]
    top = _face(m, 2, 1.0)
    u0 = np.zeros(n)
    u0[3 * top + 2] = -0.05
    tol = NEWTON_TOLERANCE
    u_ref, d_perm, d_newton, bound, it, prob = _newton_tolerances(oracle, kind, op, obs, top, np.zeros(n), u0, tol)
    u, res = _device_newton(engine, kind, op, obs, top, np.zeros(n), u0, tol)
    print(f"pressed {kind} {op}: reference {it} iterations, device {res.iterations}; d_perm {d_perm:.2e} d_newton {d_newton:.2e}; "
          f"active nodes {(cr.gap(obs, m.vertices, u_ref) < 0).sum()}; kernel {engine.last_kernel_name()}")
    assert (cr.gap(obs, m.vertices, u_ref) < 0).sum() >= 4 and res.residual_norm <= tol
    assert (it == 1 if op == "elastic" else 3 <= it <= 4)     # (what the reference takes in this scene: quadratic convergence)
    _check("u", _rel(u, u_ref), bound)


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["elastic", "neo_hookean"])
@pytest.mark.parametrize("kind", ["HEX8", "TET4"])
def test_newton_corner(engine, oracle, kind, op):
    """(b) no Dirichlet node: three half-spaces x_a >= 0.01 hold the cube against a nodal load of -0.5 per component; the contact forces
    balance the load"""
    m = _mesh(kind)[0]
    n = m.vertices.size
    obs = [("half_space", tuple(0.01 * np.eye(3)[a]), tuple(np.eye(3)[a]), 1.0e4) for a in range(3)]
    f = np.full(n, -0.5)
    tol = NEWTON_TOLERANCE
    none = np.zeros(0, dtype=np.int64)
    u_ref, d_perm, d_newton, bound, it, prob = _newton_tolerances(oracle, kind, op, obs, none, f, np.zeros(n), tol)
    u, res = _device_newton(engine, kind, op, obs, none, f, np.zeros(n), tol)
    print(f"corner {kind} {op}: reference {it} iterations, device {res.iterations}; d_perm {d_perm:.2e} d_newton {d_newton:.2e}")
    _check("u", _rel(u, u_ref), bound)
    asm_u = _assembler(engine, kind, op, u)
    engine.set_obstacles(_fa_obstacles(obs))
    g = fa.Contact(asm_u).force().reshape(-1, 3)
    balance = np.abs(g.sum(axis=0) - f.reshape(-1, 3).sum(axis=0)).max()
    _check("sum g - sum f", balance, 10.0 * np.sqrt(n) * tol)


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["neo_hookean"])
def test_newton_ball_indenter(engine, oracle, op):
    """(c) a ball of radius 0.4 pressed 0.05 into the centre of the top face, the bottom held: the Gauss-Newton tangent"""
    kind = "HEX8_6"     # (the centre node of the top face and its four neighbours are inside the ball)
    m = _mesh(kind)[0]
    n = m.vertices.size
    obs = [("ball", (0.5, 0.5, 1.0 + 0.4 - 0.05), 0.4, 1.0e4)]
    bottom = _face(m, 2, 0.0)
    assert (cr.gap(obs, m.vertices, np.zeros(n)) < 0).sum() >= 4
    tol = 1e-9    # (1000 dofs and a penalty of 1e4: |F| has a rounding floor of some 1e-12, and d_newton needs tol / 100 to be reachable)
    u_ref, d_perm, d_newton, bound, it, prob = _newton_tolerances(oracle, kind, op, obs, bottom, np.zeros(n), np.zeros(n), tol)
    u, res = _device_newton(engine, kind, op, obs, bottom, np.zeros(n), np.zeros(n), tol)
    print(f"indenter {op}: reference {it} iterations, device {res.iterations}; d_perm {d_perm:.2e} d_newton {d_newton:.2e}; "
          f"active at the solution {(cr.gap(obs, m.vertices, u_ref) < 0).sum()}")
    assert (cr.gap(obs, m.vertices, u_ref) < 0).sum() >= 4
    _check("u", _rel(u, u_ref), bound)


# ------------------------------------------------------------------------------------------ GPU 5: dynamics
FLOOR = [("half_space", (0.0, 0.0, -0.02), (0.0, 0.0, 1.0), 2.0e3)]


def _drop_state(m):
    n = m.vertices.size
    v0 = np.zeros(n)
    v0[2::3] = -1.0
    return np.zeros(n), v0


@functools.lru_cache(maxsize=None)
def _drop_dt(kind, op):
    """half the critical step of central differences with the bottom face 0.02 inside the floor, from the reference's dense pencil"""
    from oracle import oracle as o

    o.lib()
    m = _mesh(kind)[0]
    prob = _problem(o, kind, op, FLOOR)
    u = np.zeros(prob.n)
    u[2::3] = -0.04
    w, _ = dr.dense_pencil(prob, u, True)
    free = _problem(o, kind, op)
    w0, _ = dr.dense_pencil(free, u, True)
    return 0.5 * 2.0 / np.sqrt(w[-1]), w[-1], w0[-1]


def _records(rec):
    return np.stack([rec.kinetic, rec.stored, rec.load_potential, rec.time], axis=1)


def _traj_rel(x, y):
    out = 0.0
    for p, q in zip(x[:3], y[:3]):
        out = max(out, _rel(p, q))
    for c in range(4):
        out = max(out, np.abs(x[3][:, c] - y[3][:, c]).max() / max(np.abs(y[3][:, c]).max(), 1e-300))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("kind,op", [("HEX8", "neo_hookean"), ("TET4", "elastic"), ("TET10", "neo_hookean")])
def test_dropped_cube_central_differences(engine, oracle, kind, op):
    """v_0 = (0, 0, -1) over the floor z >= -0.02, k = 2e3: 64 steps with records every 8 against dr.central_difference; the stored column is
    the elastic energy plus E_c; the run repeats bit for bit as 64, 32 + 32 and 8 x 8 steps"""
    m = _mesh(kind)[0]
    dt = 1e-3 if kind == "TET10" else _drop_dt(kind, op)[0]
    u0, v0 = _drop_state(m)
    prob = _problem(oracle, kind, op, FLOOR)
    if kind == "TET10":   # (no positive row-sum lumping on Tet10: the explicit scheme is refused with or without obstacles)
        asm = _assembler(engine, kind, op)
        ti = fa.CentralDifference(asm, RHO, dt).with_obstacles(_fa_obstacles(FLOOR))
        ti.set_state(u0, v0)
        with pytest.raises(fa.DynamicsError) as e:
            ti.step(1)
        assert e.value.code == FH_UNSUPPORTED and "lumped" in str(e.value)
        return
    ref = dr.central_difference(prob, u0, v0, dt, 64, 8)
    perm = dr.central_difference(_problem(oracle, kind, op, FLOOR, perm=7), u0, v0, dt, 64, 8)
    d_perm = _traj_rel(perm, ref)
    bound = max(20.0 * d_perm, 1e-13)

    def run(chunks):
        asm = _assembler(engine, kind, op)
        ti = fa.CentralDifference(asm, RHO, dt).with_obstacles(_fa_obstacles(FLOOR))
        ti.set_state(u0, v0)
        rows = []
        for c in chunks:
            rows.append(_records(ti.step(c, 8)))
        u, v, a, _, step = ti.state()
        assert step == 64
        name = engine.last_kernel_name()
        ti.close()
        return u, v, a, np.concatenate(rows), name

    got = run([64])
    print(f"drop {kind} {op}: dt {dt:.3e}; d_perm {d_perm:.2e}; kernel {got[4]}; deepest gap {cr.gap(FLOOR, m.vertices, got[0]).min():.4f}")
    _check("trajectory", _traj_rel(got, ref), bound)
    # the stored column: elastic energy plus E_c, at a recorded state inside the floor (step 16)
    asm = _assembler(engine, kind, op)
    ti = fa.CentralDifference(asm, RHO, dt).with_obstacles(_fa_obstacles(FLOOR))
    ti.set_state(u0, v0)
    rec16 = ti.step(16, 8)
    u16 = ti.state()[0]
    ti.close()
    e_el, e_c = prob.elastic_energy(u16), prob.contact_energy(u16)
    print(f"step 16: elastic {e_el:.5f}, E_c {e_c:.5f}, stored column {rec16.stored[-1]:.5f}")
    assert e_c > 0.05 * e_el and np.array_equal(rec16.stored, got[3][:2, 1])
    _check("stored = elastic + E_c", abs(rec16.stored[-1] - (e_el + e_c)) / (e_el + e_c), bound)
    for chunks in ([32, 32], [8] * 8):
        again = run(chunks)
        for p, q in zip(got[:4], again[:4]):
            assert np.array_equal(p, q), chunks


@pytest.mark.gpu
def test_dropped_cube_energy_and_rebound(engine, oracle):
    """400 steps: kinetic plus stored energy (with E_c) drifts on the device by at most twice what it drifts in the reference, and the cube
    comes back up"""
    kind, op = "HEX8", "neo_hookean"
    m = _mesh(kind)[0]
    dt = _drop_dt(kind, op)[0]
    u0, v0 = _drop_state(m)
    prob = _problem(oracle, kind, op, FLOOR)
    ref = dr.central_difference(prob, u0, v0, dt, 400, 8)
    tot_ref = ref[3][:, 0] + ref[3][:, 1]
    e0 = 0.5 * float(np.sum(prob.lumped() * v0 ** 2))
    drift_ref = np.abs(tot_ref - e0).max() / e0
    asm = _assembler(engine, kind, op)
    ti = fa.CentralDifference(asm, RHO, dt).with_obstacles(_fa_obstacles(FLOOR))
    ti.set_state(u0, v0)
    rec = ti.step(400, 8)
    u, v, _, _, _ = ti.state()
    ti.close()
    tot = rec.kinetic + rec.stored
    drift = np.abs(tot - e0).max() / e0
    print(f"energy drift: reference {drift_ref:.4f}, device {drift:.4f}; mean v_z reference {ref[1][2::3].mean():+.3f}, device {v[2::3].mean():+.3f}; "
          f"largest E_c share of a record {np.max(rec.stored) / e0:.3f}")
    assert drift_ref < 0.05 and ref[1][2::3].mean() > 0.5     # the reference's scene is what the issue describes
    assert drift <= 2.0 * drift_ref
    assert v[2::3].mean() > 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["newmark", "euler"])
def test_dropped_cube_implicit(engine, oracle, scheme):
    """4 implicit steps into the floor against dr.implicit"""
    kind, op = "HEX8", "neo_hookean"
    m = _mesh(kind)[0]
    dt = 8.0 * _drop_dt(kind, op)[0]
    u0, v0 = _drop_state(m)
    tol = 1e-10

    def reference(perm, t):
        st, u, v, a, rec, done, _ = dr.implicit(_problem(oracle, kind, op, FLOOR, perm=perm), scheme, u0, v0, dt, 4, 2, tol=t)
        assert st == "ok" and done == 4
        return u, v, a, rec

    ref = reference(None, tol)
    d_perm, d_newton = _traj_rel(reference(7, tol), ref), _traj_rel(reference(None, tol / 100.0), ref)
    bound = max(20.0 * (d_perm + d_newton), 1e-13)
    assert cr.gap(FLOOR, m.vertices, ref[0]).min() < 0.0
    asm = _assembler(engine, kind, op)
    ti = (fa.Newmark if scheme == "newmark" else fa.BackwardEuler)(asm, RHO, dt)
    ti.with_newton(fa.NewtonSettings(40, tol), linear_rel_tol=1e-13).with_obstacles(_fa_obstacles(FLOOR))
    ti.set_state(u0, v0)
    rec = ti.step(4, 2)
    u, v, a, _, _ = ti.state()
    ti.close()
    print(f"{scheme}: d_perm {d_perm:.2e} d_newton {d_newton:.2e}; deepest gap {cr.gap(FLOOR, m.vertices, u).min():.4f}")
    _check(scheme, _traj_rel((u, v, a, _records(rec)), ref), bound)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["HEX8", "TET10"])
def test_first_order_with_obstacles(engine, oracle, kind):
    """RungeKuttaLegendre (4 stages, 6 steps) on M du/dt + r(u) + g(u) = 0 from a state inside the floor, against the reference's stages"""
    op = "neo_hookean"
    m = _mesh(kind)[0]
    prob = _problem(oracle, kind, op, FLOOR)
    u0 = np.zeros(prob.n)
    u0[2::3] = -0.04
    lam = _drop_dt(kind, op)[1] if kind == "HEX8" else None
    if kind == "TET10":   # (no positive row-sum lumping: refused as without obstacles)
        asm = _assembler(engine, kind, op)
        ti = fa.RungeKuttaLegendre(asm, RHO, 1e-5, stages=4).with_obstacles(_fa_obstacles(FLOOR))
        ti.set_state(u0)
        with pytest.raises(fa.DynamicsError) as e:
            ti.step(1)
        assert e.value.code == FH_UNSUPPORTED
        return
    s = 4
    dt = 0.5 * (s * s + s) / lam

    def reference(p):
        mlump = p.lumped()
        u = u0.copy()
        w1 = 2.0 / (s * s + s)
        for _ in range(6):
            y_prev2, y_prev = None, u
            L0 = None
            for j in range(1, s + 1):
                L = -p.residual(y_prev) / mlump
                if j == 1:
                    y = y_prev + w1 * dt * L
                else:
                    mu, nu = (2.0 * j - 1.0) / j, (1.0 - j) / j
                    y = mu * y_prev + nu * y_prev2 + mu * w1 * dt * L
                y_prev2, y_prev = y_prev, y
            u = y_prev
        return u

    ref = reference(prob)
    d_perm = _rel(reference(_problem(oracle, kind, op, FLOOR, perm=7)), ref)
    bound = max(20.0 * d_perm, 1e-13)
    asm = _assembler(engine, kind, op)
    ti = fa.RungeKuttaLegendre(asm, RHO, dt, stages=s).with_obstacles(_fa_obstacles(FLOOR))
    ti.set_state(u0)
    rec = ti.step(6)
    u = ti.state()[0]
    name = engine.last_kernel_name()
    ti.close()
    print(f"RKL: d_perm {d_perm:.2e}; kernel {name}")
    _check("RKL u", _rel(u, ref), bound)
    _check("RKL stored = elastic + E_c", abs(rec.stored[-1] - prob.energy(u)) / prob.energy(u), max(bound, 1e-12))
    without = _problem(oracle, kind, op)
    assert abs(prob.energy(ref) - without.energy(ref)) > 1e-6 * prob.energy(ref)      # the term shows in this state


@pytest.mark.gpu
def test_stable_dt_sees_the_obstacles(engine, oracle):
    """fh_dynamics_stable_dt with the bottom face inside the floor against dr.power_iteration: omega_max^2 is several times the free body's"""
    kind, op = "HEX8", "neo_hookean"
    m = _mesh(kind)[0]
    prob, free = _problem(oracle, kind, op, FLOOR), _problem(oracle, kind, op)
    u = np.zeros(prob.n)
    u[2::3] = -0.04
    rq, rq_free = dr.power_iteration(prob, u, 40), dr.power_iteration(free, u, 40)
    rq_perm = dr.power_iteration(_problem(oracle, kind, op, FLOOR, perm=7), u, 40)
    bound = max(20.0 * abs(rq_perm - rq) / rq, 1e-13)
    asm = _assembler(engine, kind, op)
    ti = fa.CentralDifference(asm, RHO, 1e-3).with_obstacles(_fa_obstacles(FLOOR))
    ti.set_state(u)
    om, dtc = ti.stable_dt(40)
    ti.with_obstacles(None)
    om_free, _ = ti.stable_dt(40)
    ti.close()
    print(f"omega_max^2: reference {rq:.1f} (free {rq_free:.1f}), device {om * om:.1f} (free {om_free ** 2:.1f})")
    assert rq > 2.0 * rq_free
    _check("omega_max^2", abs(om * om - rq) / rq, bound)
    _check("omega_max^2 free", abs(om_free ** 2 - rq_free) / rq_free, bound)
    assert dtc == 2.0 / om


# ------------------------------------------------------------------------------------------ GPU 6: the eigensolver
@pytest.mark.gpu
def test_eigenmodes_at_the_corner_equilibrium(engine, oracle):
    """the three lowest modes of (K(u) + B(u), M) at the corner scene's equilibrium against the reference's dense pencil; the free body has
    six zero modes there, the held one none"""
    kind, op = "HEX8", "neo_hookean"
    m = _mesh(kind)[0]
    n = m.vertices.size
    obs = [("half_space", tuple(0.01 * np.eye(3)[a]), tuple(np.eye(3)[a]), 1.0e4) for a in range(3)]
    f = np.full(n, -0.5)
    none = np.zeros(0, dtype=np.int64)
    u_eq = _newton_tolerances(oracle, kind, op, obs, none, f, np.zeros(n), 1e-10)[0]
    prob = _problem(oracle, kind, op, obs)
    w, _ = dr.dense_pencil(prob, u_eq, False)
    w_perm, _ = dr.dense_pencil(_problem(oracle, kind, op, obs, perm=7), u_eq, False)
    w_free, _ = dr.dense_pencil(_problem(oracle, kind, op), np.zeros(n), False)
    assert np.abs(w_free[:6]).max() <= 1e-9 * w_free[6] and w[0] > 1e-3 * w[6]
    asm = _assembler(engine, kind, op, u_eq)
    es = fa.MatrixFreeEigensolver(asm, RHO).with_obstacles(_fa_obstacles(obs))
    res = es.solve(3, tol=1e-10, max_iter=400)
    theta = np.asarray(res.values)
    bound = max(20.0 * _rel(w_perm[:3], w[:3]), 1e-10)    # (the solver's tolerance: a residual of 1e-10 relative moves an eigenvalue by no more)
    print(f"theta {theta}, reference {w[:3]}")
    _check("theta", _rel(theta, w[:3]), bound)


# ------------------------------------------------------------------------------------------ GPU 7: the routes off the tiles, penetrating
# (k_contact_force behind the ordered node sums of r(u), then k_newton_combine, k_dynamics_rhs, k_theta_load, k_dynamics_update and
# k_first_order_update: Tet10, and Hex8 under a rule-set table, whose row-sum lumped mass is positive, for the explicit schemes)
def _inside_floor(m):
    u = np.zeros(m.vertices.size)
    u[2::3] = -0.04      # the bottom face 0.02 inside FLOOR
    return u


@pytest.mark.gpu
def test_newton_pressed_block_off_the_tiles(engine, oracle):
    """scene (a) on Tet10: the residual through k_residual_elements, k_contact_force and k_newton_combine, the tangent through k_contact_apply"""
    kind, op = "TET10", "neo_hookean"
    m = _mesh(kind)[0]
    n = m.vertices.size
    obs = [("half_space", (0.0, 0.0, 0.02), (0.0, 0.0, 1.0), 1.0e4)]
    top = _face(m, 2, 1.0)
    u0 = np.zeros(n)
    u0[3 * top + 2] = -0.05
    tol = NEWTON_TOLERANCE
    u_ref, d_perm, d_newton, bound, it, prob = _newton_tolerances(oracle, kind, op, obs, top, np.zeros(n), u0, tol)
    u, res = _device_newton(engine, kind, op, obs, top, np.zeros(n), u0, tol)
    name = engine.last_kernel_name()
    print(f"pressed {kind} {op}: reference {it} iterations, device {res.iterations}; d_perm {d_perm:.2e} d_newton {d_newton:.2e}; "
          f"active nodes {(cr.gap(obs, m.vertices, u_ref) < 0).sum()}; kernel {name}")
    assert name == "k_residual_elements + k_vector_from_elements_soa + k_contact_force + k_newton_combine", name
    assert (cr.gap(obs, m.vertices, u_ref) < 0).sum() >= 4 and res.residual_norm <= tol
    _check("u", _rel(u, u_ref), bound)


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["newmark", "theta"])
def test_implicit_steps_off_the_tiles_from_inside_the_floor(engine, oracle, scheme):
    """Tet10 from a state with the bottom face inside the floor: Newmark (a_0 through k_dynamics_rhs on r + g) and the theta method with
    theta = 1/2 (its load through k_theta_load on r + g), 2 steps each, against the reference"""
    kind, op = "TET10", "neo_hookean"
    m = _mesh(kind)[0]
    u0 = np.zeros(m.vertices.size)
    u0[2::3] = -0.022     # the bottom face 0.002 inside FLOOR: a push the Neo-Hookean body takes without inverting
    z = np.zeros_like(u0)
    dt = 2e-3 if scheme == "newmark" else 2e-5     # (the gradient flow with density 1 is stiff: its step is short)
    tol = 1e-10
    assert (cr.gap(FLOOR, m.vertices, u0) < 0).sum() >= 9

    def theta_reference(prob, t):
        M, u, th = prob.mass(), u0.copy(), 0.5
        for _ in range(2):
            load = -(1.0 - th) / th * prob.residual(u)
            un = u.copy()
            st, u, _ = dr.newton(prob, lambda x: M @ (x - un) + th * dt * (prob.residual(x) - load), lambda x: (M + th * dt * prob.tangent(x)).tocsr(),
                                 u.copy(), t)
            assert st == "ok"
        return (u,)

    def reference(perm, t):
        prob = _problem(oracle, kind, op, FLOOR, perm=perm)
        if scheme == "theta":
            return theta_reference(prob, t)
        st, u, v, a, rec, done, _ = dr.implicit(prob, "newmark", u0, z, dt, 2, 1, tol=t)
        assert st == "ok" and done == 2
        return u, v, a

    ref = reference(None, tol)
    d_perm = max(_rel(p, q) for p, q in zip(reference(7, tol), ref))
    d_newton = max(_rel(p, q) for p, q in zip(reference(None, tol / 100.0), ref))
    bound = max(20.0 * (d_perm + d_newton), 1e-13)
    asm = _assembler(engine, kind, op)
    if scheme == "theta":
        ti = fa.ThetaMethod(asm, RHO, dt, theta=0.5)
    else:
        ti = fa.Newmark(asm, RHO, dt)
    ti.with_newton(fa.NewtonSettings(40, tol), linear_rel_tol=1e-13).with_obstacles(_fa_obstacles(FLOOR))
    ti.set_state(u0)
    ti.step(2, 1)
    state = ti.state()
    got = (state[0],) if scheme == "theta" else state[:3]
    ti.close()
    print(f"{scheme} off the tiles: d_perm {d_perm:.2e} d_newton {d_newton:.2e}")
    for name, p, q in zip("uva", got, ref):
        _check(f"{scheme} {name}", _rel(p, q), bound)
    # the floor pushes the body up: without it the same steps end elsewhere
    without = _problem(oracle, kind, op)
    if scheme == "newmark":
        st, u_free, *_ = dr.implicit(without, "newmark", u0, z, dt, 2, 1, tol=tol)
        assert _rel(u_free, ref[0]) > 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["central", "rkl"])
def test_explicit_steps_off_the_tiles(engine, oracle, scheme):
    """Hex8 under a rule-set table (no tiles; the lumped mass is positive): central differences into the floor through k_dynamics_update and
    Runge-Kutta-Legendre from inside it through k_first_order_update, both on r + g of k_contact_force"""
    kind, op = "HEX8", "neo_hookean"
    m = _mesh(kind)[0]
    qt, groups = _rule_set(kind)
    dt = _drop_dt(kind, op)[0]
    u0, v0 = _drop_state(m)

    def reference(perm):
        prob = _problem(oracle, kind, op, FLOOR, perm=perm, groups=groups)
        if scheme == "central":
            u, v, a, rec = dr.central_difference(prob, u0, v0, dt, 16, 8)
            return u, v, a, rec[:, 1]
        mlump, u = prob.lumped(), _inside_floor(m)
        s, h = 4, 0.5 * 20.0 / _drop_dt(kind, op)[1]
        w1 = 2.0 / (s * s + s)
        for _ in range(3):
            y2, y1 = None, u
            for j in range(1, s + 1):
                L = -prob.residual(y1) / mlump
                mu, nu = (2.0 * j - 1.0) / j, (1.0 - j) / j
                y = y1 + w1 * h * L if j == 1 else mu * y1 + nu * y2 + mu * w1 * h * L
                y2, y1 = y1, y
            u = y1
        return u, np.array([prob.energy(u)])

    ref = reference(None)
    d_perm = max(_rel(p, q) for p, q in zip(reference(7), ref))
    bound = max(20.0 * d_perm, 1e-13)
    asm = _assembler(engine, kind, op, qt=qt)
    if scheme == "central":
        ti = fa.CentralDifference(asm, RHO, dt).with_obstacles(_fa_obstacles(FLOOR))
        ti.set_state(u0, v0)
        rec = ti.step(16, 8)
        name = "k_residual_elements + k_vector_from_elements_soa + k_contact_force + k_dynamics_update"
        u, v, a, _, _ = ti.state()
        got = (u, v, a, rec.stored)
        assert cr.gap(FLOOR, m.vertices, u).min() < 0.0
    else:
        ti = fa.RungeKuttaLegendre(asm, RHO, 0.5 * 20.0 / _drop_dt(kind, op)[1], stages=4).with_obstacles(_fa_obstacles(FLOOR))
        ti.set_state(_inside_floor(m))
        rec = ti.step(3)
        name = "k_residual_elements + k_vector_from_elements_soa + k_contact_force + k_first_order_update"
        got = (ti.state()[0], rec.stored[-1:])
    ti.close()
    print(f"{scheme} off the tiles: d_perm {d_perm:.2e}")
    for i, (p, q) in enumerate(zip(got, ref)):
        _check(f"{scheme} [{i}]", _rel(p, q), bound)
    # the name of what ran: the step's launch, read before a record's energy pass replaces it
    asm2 = _assembler(engine, kind, op, qt=qt)
    if scheme == "central":
        t2 = fa.CentralDifference(asm2, RHO, dt).with_obstacles(_fa_obstacles(FLOOR))
        t2.set_state(u0, v0)
    else:
        t2 = fa.RungeKuttaLegendre(asm2, RHO, 1e-6, stages=1).with_obstacles(_fa_obstacles(FLOOR))
        t2.set_state(_inside_floor(m))
    t2.state()      # (forms a_0 / the rate: one residual evaluation and the update kernel, no record)
    assert engine.last_kernel_name() == name, engine.last_kernel_name()
    t2.close()


# ------------------------------------------------------------------------------------------ GPU 8: whose obstacles the engine holds
@pytest.mark.gpu
def test_obstacles_are_handed_over_again_after_the_engine_was_given_a_mesh(engine):
    """an object's obstacles are its own: a second assembler built on the engine (fh_set_mesh clears the engine's obstacles) between two
    uses leaves the term in place; an object that was never given obstacles does not solve with another object's; obstacles set on the
    engine directly belong to no object and stay"""
    kind, op = "HEX8", "neo_hookean"
    m = _mesh(kind)[0]
    n = m.vertices.size
    obs = _fa_obstacles(_three_kinds(3))
    u = _random_u(m)
    x = np.random.default_rng(20).uniform(-1.0, 1.0, n)
    asm = _assembler(engine, kind, op, u)
    owner = fa.MatrixFreeTangent(asm).with_obstacles(obs)
    with_term = owner.apply(np.zeros(n), x).copy()
    plain = fa.MatrixFreeTangent(asm)
    without = plain.apply(np.zeros(n), x).copy()          # never given obstacles: not the owner's
    assert not np.array_equal(with_term, without) and fa.Contact(engine).energy() == 0.0
    assert np.array_equal(owner.apply(np.zeros(n), x), with_term)       # handed over again
    asm_b = _assembler(engine, kind, op, u)               # the engine is given the mesh again: its obstacles are gone
    assert fa.Contact(engine).energy() == 0.0
    assert np.array_equal(owner.apply(np.zeros(n), x), with_term) and fa.Contact(engine).energy() > 0.0
    # the same for the solver objects: Newton with and without the term, around a rebuilt assembler
    top = _face(m, 2, 1.0)
    floor = _fa_obstacles([("half_space", (0.0, 0.0, 0.02), (0.0, 0.0, 1.0), 1.0e4)])
    u0 = np.zeros(n)
    u0[3 * top + 2] = -0.05
    asm_c = _assembler(engine, kind, op)
    newton = fa.MatrixFreeNewton(asm_c).with_dirichlet_nodes(top).with_obstacles(floor)
    first = u0.copy()
    newton.solve(first, fa.NewtonSettings(40, 1e-10), linear_rel_tol=1e-12)
    asm_d = _assembler(engine, kind, op)
    second = u0.copy()
    newton.solve(second, fa.NewtonSettings(40, 1e-10), linear_rel_tol=1e-12)
    bottom = _face(m, 2, 0.0)
    assert np.array_equal(first, second) and first[3 * bottom + 2].min() > 0.015     # held up by the floor at z = 0.02, less the penetration
    free = u0.copy()
    fa.MatrixFreeNewton(asm_d).with_dirichlet_nodes(top).solve(free, fa.NewtonSettings(40, 1e-10), linear_rel_tol=1e-12)
    assert free[3 * bottom + 2].max() < -0.04 and fa.Contact(engine).energy() == 0.0    # no floor: the block moves down with its top face
    # obstacles set on the engine itself stay for objects that own none
    engine.set_obstacles(floor)
    kept = u0.copy()
    fa.MatrixFreeNewton(asm_d).with_dirichlet_nodes(top).solve(kept, fa.NewtonSettings(40, 1e-10), linear_rel_tol=1e-12)
    assert _rel(kept, first) <= 1e-12
    assert asm_b is not None


@pytest.mark.gpu
def test_kernel_names_and_the_stand_alone_v_cycle(engine):
    """fh_last_kernel_name after the diagonal with B; the name does not grow over applications without an element to run; fh_mg_apply_dev
    with obstacles set is refused"""
    import torch

    kind, op = "TET10", "neo_hookean"
    m = _mesh(kind)[0]
    n = m.vertices.size
    asm = _assembler(engine, kind, op, _random_u(m))
    t = fa.MatrixFreeTangent(asm).with_obstacles(_fa_obstacles(_three_kinds(3)))
    t.diagonal()
    assert engine.last_kernel_name() == "k_contact_diagonal"
    engine.set_active_elements(np.zeros(m.num_elements(), dtype=np.uint8))
    x = np.ones(n)
    names = set()
    for _ in range(3):
        t.apply(np.zeros(n), x)
        names.add(engine.last_kernel_name())
    assert len(names) == 1 and len(names.pop()) < 120
    engine.set_active_elements(None)
    # the stand-alone V-cycle
    coarse, w, p = _mesh("HEX8")
    eng = fa.Engine(0)
    try:
        fine, transfer = fa.refine_uniformly_with_transfer(coarse)
        qt = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(LAME)
        asm_f = (fa.ElementEllipticAssemblerBuilder(eng).with_finite_element_space(fine).with_operator(fa.MaterialEllipticOperator(fa.NeoHookeanMaterial()))
                 .with_quadrature_table(qt).with_u(np.zeros(fine.vertices.size)).build())
        mg = fa.GeometricMultigrid(asm_f, [coarse], [transfer])
        r = torch.ones(fine.vertices.size, dtype=torch.float64, device="cuda:0")
        z = torch.zeros_like(r)
        top = _face(fine, 2, 1.0)
        mg.apply(r, z, dirichlet_nodes=top)
        eng.set_obstacles([fa.HalfSpace((0, 0, 0.02), (0, 0, 1), 1e4)])
        assert _code(mg.apply, r, z, dirichlet_nodes=top) == FH_UNSUPPORTED
        eng.set_obstacles(None)
        mg.apply(r, z, dirichlet_nodes=top)
    finally:
        eng.close()
