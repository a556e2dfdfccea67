"""Dirichlet conditions on single displacement components (fh_set_operator_dirichlet_dofs, fh_apply_dirichlet_dofs_csr_dev / _rhs_dev,
with_dirichlet_dofs): rollers and symmetry planes on every route that honours a node set.

The host model (tests/dirichlet_dofs_reference.py) is the assembled K(u) with the rows and columns of the constrained dofs zeroed and the
scale on their diagonal.  Bounds: the maps against the model 1e-12 max|K| max|x| (the bar the matrix-free tests hold node sets to); the
uniaxial patch test 1e-9 max|u_exact| and 1e-9 |t|; the finite-strain stretch 1e-8 in u; central differences 4.8e-13 (the Hex8 constant of
tests/test_dynamics.py, TRAJECTORY_TOLERANCE) and backward Euler 10 steps kappa linear_rel_tol (its bound for the linear implicit schemes);
the eigenvalues as tests/test_eigs.py bounds them, |theta - lambda| <= ||r||_2 / sqrt(lambda_min(M_ff))."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import fenris_amd as fa
from fenris_amd import _ffi, quadrature
from fenris_amd.dirichlet import ALL_COMPONENTS, DofSet, dof_masks

import boundary_reference as br
import contact_reference as cr
import dirichlet_dofs_reference as ddr
import dynamics_reference as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FH_BAD_ARGUMENT = 2
E_MOD, NU = 1.0e6, 0.3
LAME = fa.LameParameters.from_young_poisson(fa.YoungPoisson(E_MOD, NU))
RHO = 1000.0
NEW = ("fh_set_operator_dirichlet_dofs", "fh_apply_dirichlet_dofs_csr_dev", "fh_apply_dirichlet_dofs_rhs_dev")
SHAPES = ["HEX8_2", "HEX8_3", "HEX8_7", "TET4", "QUAD4", "TRI3", "TET10"]   # TET10: off the tiles, the ordered per-element route


@pytest.fixture()
def engine():
    eng = fa.Engine(0)
    yield eng
    eng.close()


@functools.lru_cache(maxsize=None)
def _mesh(shape):
    P, T, Q = fa.procedural, quadrature.tensor, quadrature.total_order
    make = {"HEX8_2": (lambda: P.create_unit_box_uniform_hex_mesh_3d(2), T.hexahedron_gauss(2)),
            "HEX8_3": (lambda: P.create_unit_box_uniform_hex_mesh_3d(3), T.hexahedron_gauss(2)),
            "HEX8_7": (lambda: P.create_unit_box_uniform_hex_mesh_3d(7), T.hexahedron_gauss(2)),
            "HEX8_BAR": (lambda: P.create_rectangular_uniform_hex_mesh(1.0, 4, 1, 1, 1), T.hexahedron_gauss(2)),
            "TET4": (lambda: P.create_unit_box_uniform_tet_mesh_3d(2), Q.tetrahedron(2)),
            "QUAD4": (lambda: P.create_unit_square_uniform_quad_mesh_2d(4), T.quadrilateral_gauss(2)),
            "TRI3": (lambda: P.create_unit_square_uniform_tri_mesh_2d(4), Q.triangle(2)),
            "TET10": (lambda: fa.tet10_mesh_from_tet4(P.create_unit_box_uniform_tet_mesh_3d(2)), Q.tetrahedron(4))}
    gen, (w, p) = make[shape]
    return gen(), np.asarray(w), np.asarray(p)


def _operator(op):
    return {"laplace": fa.LaplaceOperator(), "elastic": fa.MaterialEllipticOperator(fa.LinearElasticMaterial()),
            "neo_hookean": fa.MaterialEllipticOperator(fa.NeoHookeanMaterial())}[op]


def _sdim(m, op):
    return 1 if op == "laplace" else m.vertices.shape[1]


def _assembler(engine, m, w, p, op, u=None, lame=LAME):
    s = _sdim(m, op)
    qt = fa.UniformQuadratureTable.from_points_and_weights(p, w)
    qt = qt if op == "laplace" else qt.with_uniform_data(lame)
    return (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(m).with_operator(_operator(op)).with_quadrature_table(qt)
            .with_u(np.zeros(s * m.num_nodes()) if u is None else u).build())


def _small_u(m, op, seed=3, size=0.01):
    return np.random.default_rng(seed).uniform(-size, size, _sdim(m, op) * m.num_nodes()) if op == "neo_hookean" else None


def _assembled(asm):
    """K(u) with device values"""
    return fa.CsrAssembler(fa.SCATTER_GATHER).assemble(asm, device_values=True)


def _scipy(csr):
    return fa.CsrMatrix(csr.row_offsets, csr.col_indices, csr.values.cpu().numpy()).to_scipy()


def _mass(m, w, p, s, rho=RHO):
    """the consistent mass, assembled on an engine of its own"""
    meng = fa.Engine(0)
    masm = (fa.ElementMassAssembler.with_solution_dim(s, meng).with_space(m)
            .with_quadrature_table(fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(fa.Density(rho))))
    M = _scipy(fa.CsrAssembler(fa.SCATTER_GATHER).assemble(masm, device_values=True))
    meng.close()
    return M


def _map(asm, op):
    return fa.MatrixFreeTangent(asm) if op == "neo_hookean" else fa.MatrixFreeOperator(asm)


def _face(m, axis, value):
    return np.where(np.isclose(m.vertices[:, axis], value))[0].astype(np.uint64)


def _rollers(obj, m, planes=(0, 1, 2)):
    """u_axis = 0 on the face axis = 0, for each axis of planes"""
    for axis in planes:
        obj.with_dirichlet_dofs(_face(m, axis, 0.0), [axis])
    return obj


def _roller_set(m, planes=(0, 1, 2)):
    ds = DofSet.of(None)
    for axis in planes:
        ds = ds.joined(_face(m, axis, 0.0), [axis])
    return ds


# ------------------------------------------------------------------------------------------ 9. without a device
def test_model_agrees_with_dense_elimination():
    """the constrained matrix of the model solves what eliminating the constrained dofs solves, on a 2^3 Hex8 cube with a mixed set"""
    X, conn, K = ddr.hex8_box_elastic(2, LAME.lambda_, LAME.mu)
    assert np.abs(K - K.T).max() <= 1e-9 * np.abs(K).max() and np.abs(K @ np.ones(len(K))).max() <= 1e-9 * np.abs(K).max()
    rng = np.random.default_rng(5)
    nodes, masks = ddr.random_mixed_set(rng, len(X), 3)
    bottom = np.where(X[:, 2] == 0.0)[0]                       # (and the bottom face clamped, so that K_ff is regular)
    nodes, masks = np.concatenate([nodes, bottom.astype(np.uint64)]), np.concatenate([masks, np.full(len(bottom), 7, dtype=np.uint8)])
    dofs = ddr.dof_list(nodes, masks, 3)
    assert 0 < len(dofs) < len(K) and len(set(masks.tolist())) >= 3
    b = rng.uniform(-1, 1, len(K))
    x_el = ddr.eliminate(K, dofs, b)
    A = ddr.constrain(K, dofs)
    assert np.abs(A - A.T).max() <= 1e-9 * np.abs(K).max() and np.all(A[dofs, dofs] == ddr.scale_of(K)) and ddr.scale_of(K) == abs(K[0, 0])
    bc = b.copy()
    bc[dofs] = 0.0
    x_model = np.linalg.solve(A, bc)
    assert np.abs(x_model - x_el).max() <= 1e-10 * np.abs(x_el).max() and np.all(x_model[dofs] == 0.0)


def test_python_argument_forms():
    """boolean array, component list, duplicates and accumulation over calls give the expected (nodes, masks) pairs"""
    n, mk = dof_masks([4, 2, 9], [0, 2])
    assert n.dtype == np.uint64 and mk.dtype == np.uint8 and n.tolist() == [4, 2, 9] and mk.tolist() == [5, 5, 5]
    n, mk = dof_masks([4, 2], np.array([[True, False, False], [False, True, True]]))
    assert n.tolist() == [4, 2] and mk.tolist() == [1, 6]
    for bad in (lambda: dof_masks([1, 2], np.array([[True, False, False], [False, False, False]])), lambda: dof_masks([1], [8]),
                lambda: dof_masks([1], []), lambda: dof_masks([1, 2], np.array([[True, False, False]])), lambda: dof_masks([1], [0.5])):
        with pytest.raises(ValueError):
            bad()
    ds = DofSet.of(None).joined([7, 3, 7], [0]).joined([3, 5], [1]).joined([5], np.array([[False, False, True]]))
    assert ds.nodes.tolist() == [3, 5, 7] and ds.masks.tolist() == [3, 6, 1]
    assert ds.dof_indices(3).tolist() == [9, 10, 16, 17, 21]
    full = DofSet.of([6, 1]).joined([1, 2], [2])           # a node set first: every component of its nodes stays held
    assert full.nodes.tolist() == [1, 2, 6] and full.masks.tolist() == [ALL_COMPONENTS, 4, ALL_COMPONENTS]
    assert full.dof_indices(2).tolist() == [2, 3, 12, 13] and full.dof_indices(3).tolist() == [3, 4, 5, 8, 18, 19, 20]
    assert ds.node_masks(9).tolist() == [0, 0, 0, 3, 0, 6, 0, 1, 0]
    coarse = ds.injected([7, 0, 5], 9)                      # coarse node j is the fine node inj[j]
    assert coarse.nodes.tolist() == [0, 2] and coarse.masks.tolist() == [1, 6]

    class Holder:   # (what every with_dirichlet_dofs does to its object, without an engine)
        _nodes = None

        def _bind(self, force=False):
            self.bound = self._nodes

    h = Holder()
    fa.dirichlet.with_dirichlet_dofs(h, [2, 0], [0])
    fa.dirichlet.with_dirichlet_dofs(h, [2], [1])
    assert h.bound is h._nodes and h._nodes.nodes.tolist() == [0, 2] and h._nodes.masks.tolist() == [1, 3]


def test_new_names_are_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "fenris_hip.h")).read()
    rust = open(os.path.join(ROOT, "bindings", "fenris_hip_sys.rs")).read()
    for name in NEW:
        assert f"int {name}(" in header and f"pub fn {name}(" in rust and name in _ffi._SIGS
    for cls in (fa.MatrixFreeOperator, fa.MatrixFreeTangent, fa.MatrixFreeShiftedTangent, fa.MatrixFreeNewton, fa.MatrixFreeEigensolver,
                fa.TimeIntegrator, fa.FirstOrderIntegrator):
        assert callable(getattr(cls, "with_dirichlet_dofs"))
    assert callable(fa.apply_homogeneous_dirichlet_dofs_csr) and callable(fa.apply_homogeneous_dirichlet_dofs_rhs)
    assert callable(fa.Engine.set_operator_dirichlet_dofs)


# ------------------------------------------------------------------------------------------ 8. arguments, through the C ABI
def _call_set(engine, nodes, masks, count=None):
    nodes = None if nodes is None else _ffi.as_u64(nodes)
    masks = None if masks is None else np.ascontiguousarray(masks, dtype=np.uint8)
    return engine._lib.fh_set_operator_dirichlet_dofs(engine._h, _ffi.up(nodes), None if masks is None else masks.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                     (0 if nodes is None else len(nodes)) if count is None else count)


@pytest.mark.gpu
def test_argument_handling(engine):
    import torch

    for name in NEW:
        assert hasattr(engine._lib, name)
    m, w, p = _mesh("HEX8_2")
    asm = _assembler(engine, m, w, p, "elastic")
    n = 3 * m.num_nodes()
    x = torch.ones(n, dtype=torch.float64, device="cuda:0")
    y = torch.empty_like(x)
    apply = lambda: (engine.apply_operator_dev(x, y), y.cpu().numpy())[1]
    free = apply()
    for nodes, masks, word in (([1, 2], [1, 0], "mask of 0"), ([1, m.num_nodes()], [1, 1], "out of range")):
        assert _call_set(engine, nodes, masks) == FH_BAD_ARGUMENT and word in engine.last_error()
    assert _call_set(engine, [1, 2], None) == FH_BAD_ARGUMENT and "null" in engine.last_error()
    assert np.array_equal(apply(), free)                                       # (a refused call changes nothing)
    assert _call_set(engine, [4, 9, 4], [1, 7, 4]) == 0                        # a duplicate node: the masks are OR-ed
    ored = apply()
    assert _call_set(engine, [4, 9], [5, 7]) == 0
    assert np.array_equal(apply(), ored) and not np.array_equal(ored, free)
    scale = float(engine_diagonal(engine, n)[12])
    assert ored[12] == scale and ored[14] == scale and ored[13] != scale and np.all(ored[27:30] == scale)
    assert _call_set(engine, None, None) == 0                                  # (NULL, NULL, 0) clears
    assert np.array_equal(apply(), free)
    assert _call_set(engine, [4], [1]) == 0
    engine.set_mesh(m)                                                         # fh_set_mesh clears
    asm = _assembler(engine, m, w, p, "elastic")
    assert np.array_equal(apply(), free)
    # a component >= S is refused when a route uses the set: Laplace with bit 1; a node set (all ones) never trips it
    leng = fa.Engine(0)
    lasm = _assembler(leng, m, w, p, "laplace")
    xs = torch.ones(m.num_nodes(), dtype=torch.float64, device="cuda:0")
    ys = torch.empty_like(xs)
    assert _call_set(leng, [3, 5], [1, 2]) == 0
    with pytest.raises(fa.FenrisError) as err:
        leng.apply_operator_dev(xs, ys)
    assert err.value.code == FH_BAD_ARGUMENT and "node 5" in str(err.value) and "component 1" in str(err.value)
    leng.set_operator_dirichlet_nodes([3, 5])
    leng.apply_operator_dev(xs, ys)
    with_nodes = ys.cpu().numpy().copy()
    assert _call_set(leng, [3, 5], [1, 1]) == 0
    leng.apply_operator_dev(xs, ys)
    assert np.array_equal(ys.cpu().numpy(), with_nodes)
    # the assembled path checks at once
    csr = _assembled(lasm)
    for nodes, masks, word in (([1], [0], "mask of 0"), ([m.num_nodes()], [1], "out of range"), ([1], [2], "component 1")):
        with pytest.raises(fa.FenrisError) as err:
            leng.apply_dirichlet_dofs_csr_dev(csr.values, nodes, masks)
        assert err.value.code == FH_BAD_ARGUMENT and word in str(err.value)
        with pytest.raises(fa.FenrisError) as err:
            leng.apply_dirichlet_dofs_rhs_dev(xs, nodes, masks)
        assert err.value.code == FH_BAD_ARGUMENT and word in str(err.value)
    leng.close()


def engine_diagonal(engine, n):
    import torch

    d = torch.empty(n, dtype=torch.float64, device="cuda:0")
    engine._check(engine._lib.fh_operator_diagonal_dev(engine._h, C.c_void_p(d.data_ptr())))
    return d.cpu().numpy()


@pytest.mark.gpu
def test_mg_create_refuses_a_coarse_mask_that_differs_in_one_bit(engine):
    meshes, ts = fa.refine_uniformly_repeat_with_transfers(fa.procedural.create_unit_box_uniform_hex_mesh_3d(2), 1)
    fine = meshes[-1]
    w, p = (np.asarray(a) for a in quadrature.tensor.hexahedron_gauss(2))
    asm = _assembler(engine, fine, w, p, "elastic")
    mg = fa.GeometricMultigrid(asm, meshes[:-1], ts)
    held = DofSet.of(None).joined(_face(fine, 0, 0.0), [0, 1])
    engine.set_operator_dirichlet_nodes(held)
    coarse = held.injected(mg._inj[0], fine.num_nodes())
    mg.levels[0].engine.set_operator_dirichlet_nodes(coarse)
    mg._create()                                                              # the injected masks: accepted
    mg._destroy()
    wrong = coarse.masks.copy()
    wrong[0] ^= 2
    mg.levels[0].engine.set_operator_dirichlet_nodes(DofSet(coarse.nodes, wrong))
    with pytest.raises(fa.FenrisError) as err:
        mg._create()
    assert err.value.code == FH_BAD_ARGUMENT and "a coarse node must constrain exactly the components its injected fine node does" in str(err.value)


# ------------------------------------------------------------------------------------------ 1. node sets, bit for bit
@pytest.mark.gpu
def test_node_sets_are_unchanged_bit_for_bit(engine):
    """set_operator_dirichlet_dofs(nodes, all components) against set_operator_dirichlet_nodes(nodes) on every route"""
    import torch

    meshes, ts = fa.refine_uniformly_repeat_with_transfers(fa.procedural.create_unit_box_uniform_hex_mesh_3d(2), 1)
    m = meshes[-1]
    w, p = (np.asarray(a) for a in quadrature.tensor.hexahedron_gauss(2))
    n = 3 * m.num_nodes()
    rng = np.random.default_rng(0)
    nodes = np.unique(np.concatenate([_face(m, 0, 0.0), rng.permutation(m.num_nodes())[:9].astype(np.uint64)]))
    x, u0 = rng.uniform(-1, 1, n), rng.uniform(-0.01, 0.01, n)
    f = np.zeros(n)
    f[0::3] = 5.0

    def routes(by_dof):
        held = (lambda o: o.with_dirichlet_dofs(nodes, [0, 1, 2])) if by_dof else (lambda o: o.with_dirichlet_nodes(nodes))
        out = {}
        lin = _assembler(engine, m, w, p, "elastic")
        op = held(fa.MatrixFreeOperator(lin))
        out["apply"], out["diagonal"] = op.apply(np.zeros(n), x).tobytes(), op.diagonal().tobytes()
        mg = fa.GeometricMultigrid(lin, meshes[:-1], ts)
        r, z = torch.from_numpy(x).cuda(), torch.zeros(n, dtype=torch.float64, device="cuda:0")
        mg.apply(r, z, dirichlet_nodes=DofSet.of(None).joined(nodes, [0, 1, 2]) if by_dof else nodes)
        out["vcycle"] = z.cpu().numpy().tobytes()
        ti = held(fa.CentralDifference(lin, RHO, 1e-5)).with_load(f)
        ti.set_state(u0)
        ti.step(5)
        out["central"] = b"".join(a.tobytes() for a in ti.state()[:3])
        non = _assembler(engine, m, w, p, "neo_hookean", u0)
        tan = held(fa.MatrixFreeTangent(non))
        out["tangent"] = tan.apply(np.zeros(n), x).tobytes()
        sh = held(fa.MatrixFreeShiftedTangent(non, RHO, 1.0, 1e-4))
        out["shifted"] = sh.apply(np.zeros(n), x).tobytes() + sh.diagonal().tobytes()
        u = u0.copy()
        try:
            res = held(fa.MatrixFreeNewton(non)).with_load(f).solve(u, fa.NewtonSettings(2, 1e-30))
        except fa.MaximumIterationsReached as err:
            res = err.result
        out["newton"] = np.array([res.initial_residual_norm, res.residual_norm]).tobytes() + u.tobytes()
        return out

    a, b = routes(False), routes(True)
    for key in a:
        assert a[key] == b[key], key


# ------------------------------------------------------------------------------------------ 2. the map is the constrained matrix
@pytest.mark.gpu
@pytest.mark.parametrize("op", ["laplace", "elastic", "neo_hookean"])
@pytest.mark.parametrize("shape", SHAPES)
def test_the_map_is_the_constrained_matrix(engine, shape, op):
    import torch

    m, w, p = _mesh(shape)
    s = _sdim(m, op)
    n = s * m.num_nodes()
    u = _small_u(m, op)
    asm = _assembler(engine, m, w, p, op, u)
    rng = np.random.default_rng(11)
    nodes, masks = ddr.random_mixed_set(rng, m.num_nodes(), s)
    comps = ((masks[:, None] >> np.arange(s)) & 1).astype(bool)
    dofs = ddr.dof_list(nodes, masks, s)
    assert s == 1 or len({int(c.sum()) for c in comps}) == min(s, 3)            # fully, one and (3-D) two components
    csr = _assembled(asm)
    K = _scipy(csr)
    A = ddr.constrain(K, dofs)
    kmax = np.abs(K).max()
    x = rng.uniform(-1, 1, n)
    bound = 1e-12 * kmax * np.abs(x).max()
    op_ = _map(asm, op).with_dirichlet_dofs(nodes, comps)
    y = op_.apply(np.zeros(n), x)
    d = op_.diagonal()
    print(f"{shape} {op}: apply {np.abs(y - A @ x).max():.3e}, diagonal {np.abs(d - np.diag(A)).max():.3e} (bound {bound:.3e})")
    assert np.abs(y - A @ x).max() <= bound and np.abs(d - np.diag(A)).max() <= 1e-12 * kmax
    # (the matrix-free scale comes from the matrix-free diagonal: the assembled one to rounding, and one value on every constrained dof)
    assert np.all(d[dofs] == d[dofs[0]]) and np.array_equal(y[dofs], d[dofs[0]] * x[dofs])
    # the shifted map alpha M + beta K(u)
    alpha, beta = 3.0, 0.7
    Sh = alpha * _mass(m, w, p, s) + beta * K
    Ash = ddr.constrain(Sh, dofs)
    sh = fa.MatrixFreeShiftedTangent(asm, RHO, alpha, beta).with_dirichlet_dofs(nodes, comps)
    ys, dsh = sh.apply(np.zeros(n), x), sh.diagonal()
    bsh = 1e-12 * np.abs(Sh).max() * np.abs(x).max()
    print(f"{shape} {op}: shifted apply {np.abs(ys - Ash @ x).max():.3e}, diagonal {np.abs(dsh - np.diag(Ash)).max():.3e} (bound {bsh:.3e})")
    assert np.abs(ys - Ash @ x).max() <= bsh and np.abs(dsh - np.diag(Ash)).max() <= 1e-12 * np.abs(Sh).max()
    # the assembled path
    fa.apply_homogeneous_dirichlet_dofs_csr(csr, nodes, comps, asm)
    got = _scipy(csr).toarray()
    assert np.abs(got - A).max() <= 1e-12 * kmax and np.all(got[A == 0.0] == 0.0) and np.all(got[dofs, dofs] == ddr.scale_of(K))
    assert np.array_equal(got[np.ix_(np.setdiff1d(np.arange(n), dofs),) * 2], K.toarray()[np.ix_(np.setdiff1d(np.arange(n), dofs),) * 2])
    # the right-hand side: exactly the masked entries, on the device and on the host
    rhs = torch.from_numpy(x.copy()).cuda()
    fa.apply_homogeneous_dirichlet_dofs_rhs(rhs, nodes, comps, asm)
    want = x.copy()
    want[dofs] = 0.0
    host = x.copy()
    fa.apply_homogeneous_dirichlet_dofs_rhs(host, nodes, comps, asm)
    assert np.array_equal(rhs.cpu().numpy(), want) and np.array_equal(host, want)


# ------------------------------------------------------------------------------------------ 3. uniaxial stress patch test
def _patch_problem(engine, m, w, p, t):
    asm = _assembler(engine, m, w, p, "elastic")
    right = m.find_boundary_faces().select(lambda c, nrm: c[:, 0] > 1.0 - 1e-9)
    f = fa.SurfaceLoad(m, right, br.face_rule(br.FACE_KIND[m.elem_kind], 2)).with_traction(np.array([t, 0.0, 0.0])).assemble_vector().reshape(-1)
    X = m.vertices
    exact = np.stack([t * X[:, 0] / E_MOD, -NU * t * X[:, 1] / E_MOD, -NU * t * X[:, 2] / E_MOD], axis=1).reshape(-1)
    return asm, f, exact


def _check_patch(engine, u, exact, t, what, expect=True):
    err = np.abs(u - exact).max() / np.abs(exact).max()
    engine.set_u(u)
    sig = fa.Recovery(engine).cauchy_stress("elements")
    sig = (sig.cpu().numpy() if hasattr(sig, "cpu") else np.asarray(sig)).reshape(-1, 3, 3)
    serr = np.abs(sig - np.diag([t, 0.0, 0.0])).max() / abs(t)
    print(f"{what}: |u - u_exact| / max|u_exact| = {err:.3e}, |sigma - diag(t, 0, 0)| / |t| = {serr:.3e}")
    if expect:
        assert err <= 1e-9 and serr <= 1e-9, (what, err, serr)
    else:
        assert err > 1e-9 and serr > 1e-9, (what, err, serr)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["HEX8_3", "TET4"])
def test_uniaxial_stress_patch(engine, shape):
    """rollers on x = 0, y = 0, z = 0 and the traction t e_x on x = 1: u = (t x / E, -nu t y / E, -nu t z / E), sigma = diag(t, 0, 0)"""
    import torch

    t = 2.5e3
    m, w, p = _mesh(shape)
    asm, f, exact = _patch_problem(engine, m, w, p, t)
    n = len(f)
    rollers = _roller_set(m)
    # matrix-free, Jacobi-PCG
    op = _rollers(fa.MatrixFreeOperator(asm), m)
    b = f.copy()
    b[rollers.dof_indices(3)] = 0.0
    u = np.zeros(n)
    op.cg_solve(b, u, preconditioner=fa.PRECOND_JACOBI, rel_tol=1e-12)
    _check_patch(engine, u, exact, t, f"{shape} Jacobi-PCG")
    # the assembled matrix through fh_apply_dirichlet_dofs_*, CG with Jacobi and with AMG
    csr = _assembled(asm)
    fa.apply_homogeneous_dirichlet_dofs_csr(csr, rollers.nodes, ((rollers.masks[:, None] >> np.arange(3)) & 1).astype(bool), asm)
    bt = torch.from_numpy(f.copy()).cuda()
    fa.apply_homogeneous_dirichlet_dofs_rhs(bt, rollers.nodes, ((rollers.masks[:, None] >> np.arange(3)) & 1).astype(bool), asm)
    assert np.array_equal(bt.cpu().numpy(), b)
    ut = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    engine.cg_solve(csr.values, bt, ut, fa.PRECOND_JACOBI, 1e-12)
    _check_patch(engine, ut.cpu().numpy(), exact, t, f"{shape} assembled, Jacobi")
    amg = fa.SmoothedAggregationAMG(asm, csr)
    ut.zero_()
    engine.cg_solve(csr.values, bt, ut, fa.PRECOND_AMG, 1e-12)
    amg.close()
    _check_patch(engine, ut.cpu().numpy(), exact, t, f"{shape} assembled, AMG")
    # the counter-check: whole nodes clamped on x = 0 suppress the Poisson contraction there, and miss the same bounds
    clamp = _face(m, 0, 0.0)
    opc = fa.MatrixFreeOperator(asm).with_dirichlet_nodes(clamp)
    bc = f.copy()
    bc[DofSet.of(clamp).dof_indices(3)] = 0.0
    uc = np.zeros(n)
    opc.cg_solve(bc, uc, preconditioner=fa.PRECOND_JACOBI, rel_tol=1e-12)
    _check_patch(engine, uc, exact, t, f"{shape} clamped on x = 0", expect=False)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["hex", "tet"])
def test_uniaxial_stress_patch_with_multigrid(engine, kind):
    """the same problem on the fine mesh of a two-level hierarchy (a refined mesh: Hex8 3^3 -> 6^3, Tet4 1 -> 2), multigrid-PCG; the masks
    go down the hierarchy by injection"""
    t = 2.5e3
    P = fa.procedural
    base = P.create_unit_box_uniform_hex_mesh_3d(3) if kind == "hex" else P.create_unit_box_uniform_tet_mesh_3d(1)
    meshes, ts = fa.refine_uniformly_repeat_with_transfers(base, 1)
    assert len(meshes) == 2
    m = meshes[-1]
    w, p = (np.asarray(a) for a in (quadrature.tensor.hexahedron_gauss(2) if kind == "hex" else quadrature.total_order.tetrahedron(2)))
    asm, f, exact = _patch_problem(engine, m, w, p, t)
    mg = fa.GeometricMultigrid(asm, meshes[:-1], ts)
    op = _rollers(fa.MatrixFreeOperator(asm), m).with_multigrid(mg)
    b = f.copy()
    b[_roller_set(m).dof_indices(3)] = 0.0
    u = np.zeros(len(f))
    it = op.cg_solve(b, u, rel_tol=1e-12)
    print(f"{kind}: {it} multigrid-PCG iterations")
    _check_patch(engine, u, exact, t, f"{kind} multigrid-PCG")


# ------------------------------------------------------------------------------------------ 4. finite-strain stretch through Newton
@pytest.mark.gpu
def test_finite_strain_uniaxial_stretch(engine):
    """NeoHookean cube on three roller planes, u_x = 0.2 prescribed on x = 1 (held from the guess): F = diag(1.2, l2, l2) with P_22 = 0"""
    m, w, p = _mesh("HEX8_2")
    lame = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1.0e3, 0.3))
    mu, lam = lame.as_pair()
    l1 = 1.2
    l2 = ddr.neo_hookean_lateral_stretch(l1, mu, lam)
    assert 0.9 < l2 < 1.0
    X = m.vertices
    exact = np.stack([(l1 - 1.0) * X[:, 0], (l2 - 1.0) * X[:, 1], (l2 - 1.0) * X[:, 2]], axis=1).reshape(-1)
    u = np.zeros(3 * m.num_nodes())
    pulled = _face(m, 0, 1.0)
    u[3 * pulled.astype(np.int64)] = l1 - 1.0
    asm = _assembler(engine, m, w, p, "neo_hookean", u, lame)
    newton = _rollers(fa.MatrixFreeNewton(asm), m).with_dirichlet_dofs(pulled, [0])
    tol = 1e-9
    res = newton.solve(u, fa.NewtonSettings(50, tol), linear_rel_tol=1e-10)
    err = np.abs(u - exact).max()
    print(f"Newton: {res.iterations} iterations, ||F|| = {res.residual_norm:.3e}, |u - u_exact| = {err:.3e}, lateral stretch {l2:.9f}")
    assert res.residual_norm <= tol and err <= 1e-8
    held = _roller_set(m).joined(pulled, [0]).dof_indices(3)
    engine.set_u(u)
    r = fa.VectorAssembler().assemble_vector(asm)
    r = (r.cpu().numpy() if hasattr(r, "cpu") else np.asarray(r)).reshape(-1)
    free = np.setdiff1d(np.arange(len(u)), held)
    print(f"|r| on the free dofs {np.linalg.norm(r[free]):.3e}, largest reaction {np.abs(r[held]).max():.3e}")
    assert np.linalg.norm(r[free]) <= tol and np.abs(r[held]).max() > 1.0     # the reactions live on the held dofs


# ------------------------------------------------------------------------------------------ 5. integrators
def _dynamics_case(engine):
    m, w, p = _mesh("HEX8_2")
    asm = _assembler(engine, m, w, p, "elastic")
    n = 3 * m.num_nodes()
    K, M = _scipy(_assembled(asm)), _mass(m, w, p, 3)
    planes = (0, 2)                                               # rollers on x = 0 and z = 0
    fixed = _roller_set(m, planes).dof_indices(3)
    f = np.zeros(n)
    f[3 * _face(m, 0, 1.0).astype(np.int64)] = 2.0e4
    f[3 * _face(m, 0, 1.0).astype(np.int64) + 1] = 0.5e4
    lf = np.linspace(0.0, 1.0, 8)
    lumped = np.asarray(M @ np.ones(n)).reshape(-1)
    fr = np.setdiff1d(np.arange(n), fixed)
    lam_max = np.linalg.eigvalsh(K.toarray()[np.ix_(fr, fr)] / np.sqrt(np.outer(lumped[fr], lumped[fr])))[-1]
    dt = 0.5 * 2.0 / np.sqrt(lam_max)
    return m, asm, K, M, planes, fixed, f, lf, dt


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["central", "euler"])
def test_integrators_against_the_stepping_model(engine, scheme):
    m, asm, K, M, planes, fixed, f, lf, dt = _dynamics_case(engine)
    n = len(f)
    rng = np.random.default_rng(2)
    u0 = rng.uniform(-1e-3, 1e-3, n)                              # (the constrained dofs start away from zero and must stay there)
    prob = ddr.LinearProblem(K, M, fixed, f, lf)
    tol_n = 1e-11 * np.linalg.norm(f) * dt * dt

    def make():
        ti = fa.CentralDifference(asm, RHO, dt) if scheme == "central" else fa.BackwardEuler(asm, RHO, dt).with_newton(
            fa.NewtonSettings(None, tol_n), linear_rel_tol=1e-12)
        return _rollers(ti, m, planes).with_load(f, lf)

    if scheme == "central":
        ref = dr.central_difference(prob, u0, np.zeros(n), dt, 8)[:3]
        tol = 4.8e-13
    else:
        st, ur, vr, ar, _, done, _ = dr.implicit(prob, "euler", u0, np.zeros(n), dt, 8, tol=tol_n)
        assert st == "ok" and done == 8
        ref = (ur, vr, ar)
        fr = prob.free
        tol = 10.0 * 8 * np.linalg.cond((M + dt * dt * K).toarray()[np.ix_(fr, fr)]) * 1e-12
    ti = make()
    ti.set_state(u0)
    ti.step(8)
    u, v, a = ti.state()[:3]
    for name, got, want in zip("uva", (u, v, a), ref):
        err = np.abs(got - want).max() / np.abs(want).max()
        print(f"{scheme} {name}: {err:.3e} (tol {tol:.3e})")
        assert err <= tol, (scheme, name, err, tol)
    assert np.array_equal(u[fixed], u0[fixed]) and not v[fixed].any() and not a[fixed].any()
    free_of_roller = 3 * _face(m, 0, 0.0).astype(np.int64) + 1    # u_y on the face x = 0 is free
    assert np.abs(u[free_of_roller] - u0[free_of_roller]).min() > 0.0
    cut = make()
    cut.set_state(u0)
    cut.step(3)
    cut.step(5)
    assert all(np.array_equal(x, y) for x, y in zip(cut.state()[:3], (u, v, a)))


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["central", "euler"])
def test_boundary_motion_moves_the_constrained_component_alone(engine, scheme):
    m, asm, K, M, planes, fixed, f, lf, dt = _dynamics_case(engine)
    n = len(f)
    top = _face(m, 2, 1.0).astype(np.int64)
    factor = np.array([0.0, 0.1, 0.3, 0.6, 1.0, 1.0, 0.8, 0.7, 0.7])
    direction = np.full(n, 7.0)                                   # (read on the constrained dofs only: u_x, u_y of the top face ignore it)
    direction[DofSet.of(_face(m, 2, 0.0)).dof_indices(3)] = 0.0  # (the clamped bottom face stays where it is)
    direction[3 * top + 2] = -2.0e-3
    ti = fa.CentralDifference(asm, RHO, dt) if scheme == "central" else fa.BackwardEuler(asm, RHO, dt).with_newton(
        fa.NewtonSettings(None, 1e-12), linear_rel_tol=1e-12)
    ti.with_dirichlet_dofs(_face(m, 2, 0.0), [0, 1, 2]).with_dirichlet_dofs(top, [2]).with_boundary_motion(direction, factor)
    v0 = np.zeros(n)
    v0[3 * top + 2] = (factor[1] - factor[0]) / dt * direction[3 * top + 2]
    ti.set_state(np.zeros(n), v0)
    for step in range(1, 9):
        ti.step(1)
        u = ti.state()[0]
        assert np.array_equal(u[3 * top + 2], (factor[step] - factor[0]) * direction[3 * top + 2]), step
    assert np.abs(u[3 * top]).max() > 0.0 and np.abs(u[3 * top + 1]).max() > 0.0 and np.abs(u).max() < 1.0
    assert not u[DofSet.of(_face(m, 2, 0.0)).dof_indices(3)].any()


@pytest.mark.gpu
def test_forward_euler_laplace_bit_masks_equal_the_node_set(engine):
    m, w, p = _mesh("HEX8_3")
    asm = _assembler(engine, m, w, p, "laplace")
    cold = _face(m, 0, 0.0)
    q = np.ones(m.num_nodes())
    u0 = np.random.default_rng(4).uniform(0, 1, m.num_nodes())
    out = []
    for by_dof in (False, True):
        ti = fa.ForwardEuler(asm, RHO, 1e-3)
        ti = ti.with_dirichlet_dofs(cold, [0]) if by_dof else ti.with_dirichlet_nodes(cold)
        ti.with_load(q).set_state(u0)
        ti.step(6)
        out.append(b"".join(np.asarray(a).tobytes() for a in ti.state()[:2]))
    assert out[0] == out[1]


# ------------------------------------------------------------------------------------------ 6. eigenmodes
@pytest.mark.gpu
def test_axial_modes_of_a_bar(engine):
    """u_y = u_z = 0 on every node of a 4 x 1 x 1 bar: the eigenproblem of the u_x dofs alone"""
    m, w, p = _mesh("HEX8_BAR")
    asm = _assembler(engine, m, w, p, "elastic")
    n = 3 * m.num_nodes()
    allnodes = np.arange(m.num_nodes(), dtype=np.uint64)
    fixed = DofSet.of(None).joined(allnodes, [1, 2]).dof_indices(3)
    free = np.setdiff1d(np.arange(n), fixed)
    assert np.array_equal(free, 3 * np.arange(m.num_nodes()))
    Kf = _scipy(_assembled(asm)).toarray()[np.ix_(free, free)]
    Mf = _mass(m, w, p, 3).toarray()[np.ix_(free, free)]
    L = np.linalg.cholesky(Mf)
    lam = np.linalg.eigvalsh(np.linalg.solve(L, np.linalg.solve(L, Kf).T))
    shift = 0.1 * lam[1]                                          # (u_x free everywhere: the rigid translation is a zero mode)
    tol = 1e-8
    res = fa.MatrixFreeEigensolver(asm, RHO).with_dirichlet_dofs(allnodes, [1, 2]).with_shift(shift).solve(3, tol=tol, preconditioner=fa.PRECOND_JACOBI)
    X = np.asarray(res.vectors)
    assert not X[fixed].any()
    xf = X[free]
    r = Kf @ xf - (Mf @ xf) * res.values
    bound = np.linalg.norm(r, axis=0) / np.sqrt(np.linalg.eigvalsh(Mf)[0]) + 1e-12 * lam[2]
    print("theta", res.values, "lambda", lam[:3], "bound", bound)
    crit = tol * (np.abs(res.values) + shift) * np.linalg.norm(Mf @ xf, axis=0) + 27 * np.finfo(float).eps * (
        np.linalg.norm(np.abs(Kf) @ np.abs(xf), axis=0) + np.abs(res.values) * np.linalg.norm(np.abs(Mf) @ np.abs(xf), axis=0))
    assert np.all(np.linalg.norm(r, axis=0) <= crit) and np.all(np.abs(res.values - lam[:3]) <= bound)
    assert np.abs(xf.T @ Mf @ xf - np.eye(3)).max() <= tol


# ------------------------------------------------------------------------------------------ 7. contact with a partly constrained node
@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["HEX8_2", "TET10"])
def test_contact_acts_on_the_free_components_of_roller_nodes(engine, shape):
    """a block pressed into a tilted floor, rollers (u_x = 0) on the face x = 0: the tangent with the contact block and the Newton residual
    are those of the host model K + B and r + g with the constrained dofs' rows and columns taken out"""
    m, w, p = _mesh(shape)
    n = 3 * m.num_nodes()
    u = np.random.default_rng(8).uniform(-0.01, 0.01, n)
    obstacles = [("half_space", (0.0, 0.0, 0.2), (-0.3, 0.0, 1.0), 2.0e5)]   # (tilted: the force has an x component)
    asm = _assembler(engine, m, w, p, "elastic", u)
    X = m.vertices
    side = _face(m, 0, 0.0)
    touching = np.where(cr.phi_table(obstacles, X, u)[0] < 0.0)[0]
    both = np.intersect1d(touching, side.astype(np.int64))
    assert len(both) >= 2 and len(touching) > len(both)
    dofs = DofSet.of(None).joined(side, [0]).dof_indices(3)
    K = _scipy(_assembled(asm))
    B = cr.tangent(obstacles, X, u)
    A = ddr.constrain(K + B, dofs, ddr.scale_of(K + B))
    floor = fa.Obstacles([fa.HalfSpace(*obstacles[0][1:])])
    x = np.random.default_rng(9).uniform(-1, 1, n)
    tan = fa.MatrixFreeTangent(asm).with_dirichlet_dofs(side, [0]).with_obstacles(floor)
    y = tan.apply(np.zeros(n), x)
    bound = 1e-12 * np.abs(K + B).max() * np.abs(x).max()
    Bd = B.toarray()
    scale = tan.diagonal()[dofs[0]]                               # (the matrix-free scale: that of the model to rounding)
    assert abs(scale - ddr.scale_of(K + B)) <= 1e-12 * np.abs(K + B).max()
    print(f"{shape}: tangent with contact {np.abs(y - A @ x).max():.3e} (bound {bound:.3e})")
    assert np.abs(y - A @ x).max() <= bound
    # present on the free components of the roller nodes, absent on the constrained one
    for nd in both:
        assert np.abs(Bd[3 * nd + 1:3 * nd + 3, 3 * nd + 1:3 * nd + 3]).max() > 0.0 and np.abs(Bd[3 * nd, 3 * nd:3 * nd + 3]).max() > 0.0
        e = np.zeros(n)
        e[3 * nd + 2] = 1.0
        col = tan.apply(np.zeros(n), e)
        assert abs(col[3 * nd + 2] - (K + B)[3 * nd + 2, 3 * nd + 2]) <= bound and col[3 * nd] == 0.0
        e[:] = 0.0
        e[3 * nd] = 1.0
        col = tan.apply(np.zeros(n), e)
        assert col[3 * nd] == scale and not col[3 * nd + 1:3 * nd + 3].any()
    # the force, through the Newton residual ||F(u_0)|| = ||(r + g) on the free dofs||
    g = cr.force(obstacles, X, u)
    F = K @ u + g
    F[dofs] = 0.0
    uu = u.copy()
    try:
        res = fa.MatrixFreeNewton(asm).with_dirichlet_dofs(side, [0]).with_obstacles(floor).solve(uu, fa.NewtonSettings(1, 1e-30))
    except fa.MaximumIterationsReached as err:
        res = err.result
    print(f"{shape}: ||F(u_0)|| {res.initial_residual_norm:.15e} model {np.linalg.norm(F):.15e}")
    assert abs(res.initial_residual_norm - np.linalg.norm(F)) <= 1e-12 * np.linalg.norm(K @ u + g)
    assert np.abs(g.reshape(-1, 3)[both, 0]).min() > 0.0            # (the model's force has an x component there: the roller takes it)
