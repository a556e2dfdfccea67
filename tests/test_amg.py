"""Smoothed-aggregation AMG (fh_amg_*, FH_PRECOND_AMG, fa.SmoothedAggregationAMG): aggregation invariants, the tentative prolongator and
near-nullspace, parity of P and A_c on every level with a NumPy restatement of the documented formulas (from the device's aggregates and
lambda), one V-cycle against a NumPy V-cycle, symmetry, positivity and bitwise repeats, AMG-PCG iteration counts under refinement, the
numeric refresh and the error contract."""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph as csg
import scipy.sparse.linalg as spla

import fenris_amd as fa
from fenris_amd import _ffi, quadrature  # noqa: F401

from amg_reference import (_key, _node_graph, _np_aggregate, _np_cheb, _np_lambda, _np_pcg, _np_vcycle, _restate, _rigid, _rowmax,  # noqa: F401
                           _tentative)

FH_BAD_ARGUMENT, FH_INVALID_STATE, FH_UNSUPPORTED = 2, 5, 6
OPS = {"laplace": fa.LaplaceOperator(), "elastic": fa.MaterialEllipticOperator(fa.LinearElasticMaterial()),
       "neo_hookean": fa.MaterialEllipticOperator(fa.NeoHookeanMaterial())}
RULES = {fa.HEX8: lambda: quadrature.tensor.hexahedron_gauss(2), fa.HEX27: lambda: quadrature.tensor.hexahedron_gauss(3),
         fa.QUAD4: lambda: quadrature.tensor.quadrilateral_gauss(2), fa.TET4: lambda: quadrature.total_order.tetrahedron(2),
         fa.TET10: lambda: quadrature.total_order.tetrahedron(4), fa.TET20: lambda: quadrature.total_order.tetrahedron(6), fa.TRI3: lambda: quadrature.total_order.triangle(2)}


@pytest.fixture()
def engine():
    eng = fa.Engine(0)
    yield eng
    eng.close()


def _mesh(name, k):
    p = fa.procedural
    if name == "hex8":
        return p.create_unit_box_uniform_hex_mesh_3d(k)
    if name == "tet4":
        return p.create_unit_box_uniform_tet_mesh_3d(k)
    if name == "tet10":
        return fa.tet10_mesh_from_tet4(p.create_unit_box_uniform_tet_mesh_3d(k))
    if name == "hex27":
        return fa.hex27_mesh_from_hex8(p.create_unit_box_uniform_hex_mesh_3d(k))
    if name == "sphere20":   # the Gmsh Tet4 sphere as Tet20, so that it coarsens (its Tet4 form has 183 nodes, 549 elastic dofs)
        return fa.tet20_mesh_from_tet4(_sphere())
    if name == "quad4":
        return p.create_unit_square_uniform_quad_mesh_2d(k)
    if name == "tri3":
        return p.create_unit_square_uniform_tri_mesh_2d(k)
    raise ValueError(name)


def _sphere():
    import os

    m = fa.io.load_msh_from_file(os.path.join(os.path.dirname(__file__), "golden", "msh", "sphere_tet4_593.msh"), fa.TET4)
    return fa.Mesh(m.vertices - m.vertices.min(axis=0), m.connectivity, m.elem_kind)


def _system(engine, m, op, clamp=True, u=None, clamp_width=1e-9):
    """(assembler, device CSR with the clamp at x = 0 applied, clamped nodes, s)"""
    d = m.vertices.shape[1]
    s = 1 if op == "laplace" else d
    w, pts = RULES[m.elem_kind]()
    qt = fa.UniformQuadratureTable.from_points_and_weights(pts, w)
    if op != "laplace":
        qt = qt.with_uniform_data(fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.3)))
    asm = (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(m).with_operator(OPS[op]).with_quadrature_table(qt)
           .with_u(np.zeros(s * m.num_nodes()) if u is None else u).build())
    csr = fa.CsrAssembler(fa.SCATTER_GATHER).assemble(asm, device_values=True)
    x0 = m.vertices[:, 0]
    nodes = np.where(x0 <= x0.min() + clamp_width * (x0.max() - x0.min()))[0].astype(np.uint64) if clamp else np.zeros(0, dtype=np.uint64)
    if len(nodes):
        engine.apply_dirichlet_csr_dev(csr.values, nodes)
    return asm, csr, nodes, s


def _rel(X, Y):
    X, Y = sp.csr_matrix(X), sp.csr_matrix(Y)
    return sp.linalg.norm(X - Y) / max(sp.linalg.norm(Y), 1e-300)


@pytest.mark.gpu
@pytest.mark.parametrize("name,k,op", [("hex8", 12, "elastic"), ("tet4", 12, "elastic"), ("quad4", 72, "laplace"), ("tri3", 72, "laplace"),
                                       ("tet10", 6, "elastic"), ("hex8", 17, "laplace"), ("sphere20", 0, "elastic")])
def test_aggregation_invariants(engine, name, k, op):
    m = _mesh(name, k)
    asm, csr, clamp, s = _system(engine, m, op, clamp_width=0.1 if name == "sphere20" else 1e-9)
    amg = fa.SmoothedAggregationAMG(asm, csr, near_nullspace="constant")
    assert amg.num_levels >= 2
    A = amg.level_matrix(0, "A")
    G = _node_graph(A, s)
    agg = amg.aggregates(0)
    isolated = np.diff(G.indptr) == 0
    assert np.array_equal(agg < 0, isolated)
    assert isolated[clamp.astype(np.int64)].all()
    nagg = agg.max() + 1
    assert np.array_equal(np.unique(agg[agg >= 0]), np.arange(nagg))   # every aggregate non-empty, ids dense
    # each aggregate is connected, and holds a node within distance 2 of all its members (its root)
    G2 = (G @ G + G).tocsr()
    for J in range(nagg):
        mem = np.where(agg == J)[0]
        sub = G[mem][:, mem]
        assert csg.connected_components(sub, directed=False)[0] == 1
        reach = (G2[mem][:, mem] + sp.identity(len(mem))).toarray() > 0
        assert reach.all(axis=1).any()
    # the documented aggregation restated on the CPU gives the same aggregates; its roots are pairwise at distance >= 3, each in its own
    # aggregate
    agg_np, roots = _np_aggregate(A, s)
    assert np.array_equal(agg, agg_np)
    assert np.array_equal(agg[roots], np.arange(nagg))
    near = G2[roots][:, roots].tocsr()
    near.setdiag(0)
    near.eliminate_zeros()
    assert near.nnz == 0
    amg2 = fa.SmoothedAggregationAMG(asm, csr, near_nullspace="constant")
    assert np.array_equal(amg2.aggregates(0), agg)
    amg2.close()
    amg.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,k,op,ns", [("hex8", 17, "laplace", "constant"), ("quad4", 52, "elastic", "rigid_body"),
                                          ("hex8", 12, "elastic", "rigid_body"), ("hex8", 12, "elastic", "user")])
def test_parity_with_numpy(engine, name, k, op, ns):
    m = _mesh(name, k)
    asm, csr, clamp, s = _system(engine, m, op)
    if ns == "user":
        rng = np.random.default_rng(5)
        B0 = np.concatenate([_rigid(m)[:, :3], rng.standard_normal((s * m.num_nodes(), 1))], axis=1)
        amg = fa.SmoothedAggregationAMG(asm, csr, near_nullspace=B0)
    else:
        B0 = _rigid(m) if ns == "rigid_body" else np.kron(np.ones((m.num_nodes(), 1)), np.eye(s))
        amg = fa.SmoothedAggregationAMG(asm, csr, near_nullspace=ns)
    levels = _restate(amg, B0)
    assert len(levels) >= 2
    for l, (A, P, T, B, Bc, agg, lam) in enumerate(levels[:-1]):
        b, nb = amg.level_info(l)["block_size"], B.shape[1]
        # the device's T and coarse B: the restatement's, orthonormal columns per aggregate, T Bc = B on aggregated nodes
        Td, Bcd = amg.level_matrix(l, "T"), amg.level_matrix(l + 1, "B").toarray()
        assert _rel(Td, T) <= 1e-12 and np.abs(Bcd - Bc).max() <= 1e-12 * max(1.0, np.abs(Bc).max())
        for J in range(0, agg.max() + 1, max(1, (agg.max() + 1) // 50)):
            rows = (b * np.where(agg == J)[0][:, None] + np.arange(b)).ravel()
            Q = Td[rows].toarray()
            G = Q.T @ Q
            keep = np.diag(G) > 0.5
            assert np.abs(G[np.ix_(keep, keep)] - np.eye(keep.sum())).max() <= 1e-12
        on = np.repeat(agg >= 0, b)
        assert np.abs((Td @ Bcd)[on] - B[on]).max() <= 1e-10 * max(1.0, np.abs(B).max())
        # lambda: the documented estimate restated, and below lambda_max(D^-1 A)
        assert abs(lam - _np_lambda(A, b, agg < 0)) <= 1e-8 * lam
        if l == 0:
            dh = 1.0 / np.sqrt(np.where(A.diagonal() != 0, A.diagonal(), np.inf))
            top = spla.eigsh(sp.diags(dh) @ A @ sp.diags(dh), k=1, which="LA", return_eigenvectors=False)[0]
            assert 0.5 * top <= lam <= top * (1 + 1e-8)
        assert _rel(amg.level_matrix(l, "P"), P) <= 1e-12, l
        Ac_dev = amg.level_matrix(l + 1, "A")
        assert _rel(Ac_dev, levels[l + 1][0]) <= 1e-12, l
        assert (Ac_dev != Ac_dev.T).nnz == 0
    # one V-cycle against the NumPy V-cycle
    import torch

    rng = np.random.default_rng(3)
    r = rng.standard_normal(s * m.num_nodes())
    z = torch.zeros(len(r), dtype=torch.float64, device="cuda")
    amg.apply(torch.from_numpy(r).cuda(), z)
    zn = _np_vcycle(levels, r)
    assert np.linalg.norm(z.cpu().numpy() - zn) <= 1e-11 * np.linalg.norm(zn)
    amg.close()


@pytest.mark.gpu
def test_symmetric_positive_repeatable(engine):
    import torch

    m = _mesh("tet4", 12)
    asm, csr, clamp, s = _system(engine, m, "elastic")
    amg = fa.SmoothedAggregationAMG(asm, csr)
    assert amg.num_levels >= 2
    n = s * m.num_nodes()
    g = torch.Generator(device="cpu").manual_seed(0)
    x, y = (torch.randn(n, generator=g, dtype=torch.float64).cuda() for _ in range(2))
    Bx, By = torch.zeros_like(x), torch.zeros_like(x)
    amg.apply(x, Bx)
    amg.apply(y, By)
    a, b = float(x @ By), float(y @ Bx)
    assert abs(a - b) <= 1e-12 * max(abs(a), abs(b))
    assert float(x @ Bx) > 0
    b_rhs = torch.ones(n, dtype=torch.float64, device="cuda")
    b_rhs[torch.from_numpy((s * clamp.astype(np.int64)[:, None] + np.arange(s)).ravel()).cuda()] = 0.0
    sols, its = [], []
    for _ in range(2):
        u = torch.zeros(n, dtype=torch.float64, device="cuda")
        its.append(engine.cg_solve(csr.values, b_rhs, u, fa.PRECOND_AMG, 1e-8))
        sols.append(u.cpu().numpy())
    assert its[0] == its[1] and np.array_equal(sols[0], sols[1])
    assert its[0] <= 40
    amg.close()


def _near_nullspace(m, s, ns):
    return _rigid(m) if ns == "rigid_body" else np.kron(np.ones((m.num_nodes(), 1)), np.eye(s))


def _np_count(A0, m, s, ns, clamp):
    """the AMG-PCG count of the NumPy restatement (aggregation, eigenvalue estimate, V-cycle and PCG all on the CPU) for the right-hand
    side 1 with the clamped rows 0"""
    levels = _restate(None, _near_nullspace(m, s, ns), A0=A0, b0=s)
    b = np.ones(A0.shape[0])
    b[(s * clamp.astype(np.int64)[:, None] + np.arange(s)).ravel()] = 0.0
    return _np_pcg(levels, b)


def _iters(engine, m, op, pre, amg_kw=None, clamp_width=1e-9, numpy_count=False):
    """(iterations of PCG to 1e-8 on the device, the NumPy restatement's count when asked for)"""
    import torch

    asm, csr, clamp, s = _system(engine, m, op, clamp_width=clamp_width)
    n = s * m.num_nodes()
    b = torch.ones(n, dtype=torch.float64, device="cuda")
    b[torch.from_numpy((s * clamp.astype(np.int64)[:, None] + np.arange(s)).ravel()).cuda()] = 0.0
    u = torch.zeros(n, dtype=torch.float64, device="cuda")
    amg, npc = None, None
    if pre == fa.PRECOND_AMG:
        amg = fa.SmoothedAggregationAMG(asm, csr, **(amg_kw or {}))
        if numpy_count:
            npc = _np_count(amg.level_matrix(0, "A"), m, s, (amg_kw or {}).get("near_nullspace", "rigid_body"), clamp)
    it = engine.cg_solve(csr.values, b, u, pre, 1e-8)
    r = (engine_spmv_residual(engine, csr, u, b))
    assert r <= 1e-7, r
    if amg is not None:
        amg.close()
    return it, npc


def engine_spmv_residual(engine, csr, u, b):
    import torch

    y = torch.zeros_like(u)
    engine.spmv(csr.values, u, y)
    return float(torch.linalg.norm(y - b) / torch.linalg.norm(b))


# AMG-PCG counts of the NumPy restatement (_np_count: aggregation, eigenvalue estimate, V-cycle and PCG on the CPU), calibrated on a CPU
# on the oracle's assembled matrices with the same clamp (scripts/calibrate_amg_bounds.py).  The device must stay within 2 of them.
BOUNDS = {("hex8", 12, "elastic"): 12, ("hex8", 24, "elastic"): 13, ("hex8", 16, "laplace"): 8, ("hex8", 32, "laplace"): 9,
          ("tet4", 12, "elastic"): 12, ("tet4", 24, "elastic"): 17, ("tet4", 16, "laplace"): 10, ("tet4", 32, "laplace"): 13}


@pytest.mark.gpu
@pytest.mark.parametrize("name,ks,op,ns", [("hex8", (12, 24, 48), "elastic", "rigid_body"), ("hex8", (16, 32, 64), "laplace", "constant"),
                                           ("tet4", (12, 24, 48), "elastic", "rigid_body"), ("tet4", (16, 32, 64), "laplace", "constant")])
def test_convergence_under_refinement(engine, name, ks, op, ns):
    """AMG-PCG counts within 2 of the NumPy restatement and of the calibrated bounds, at most 1.5x more per doubling, while Jacobi's
    about double"""
    amg_its, jac_its = [], []
    for k in ks:
        m = _mesh(name, k)
        it, npc = _iters(engine, m, op, fa.PRECOND_AMG, {"near_nullspace": ns}, numpy_count=(name, k, op) in BOUNDS)
        if npc is not None:
            print(name, k, op, "device", it, "numpy", npc)
            assert abs(it - npc) <= 2, (it, npc)
            assert it <= BOUNDS[(name, k, op)] + 2, (it, BOUNDS[(name, k, op)])
        amg_its.append(it)
        jac_its.append(_iters(engine, m, op, fa.PRECOND_JACOBI)[0])
    print(name, op, "amg", amg_its, "jacobi", jac_its)
    assert max(amg_its) <= 40, amg_its
    for a0, a1 in zip(amg_its, amg_its[1:]):
        assert a1 <= 1.5 * a0, amg_its
    assert jac_its[-1] >= 3 * jac_its[0], jac_its


@pytest.mark.gpu
@pytest.mark.parametrize("name,k,op", [("tet10", 6, "elastic"), ("hex27", 6, "elastic")])
def test_convergence_quadratic(engine, name, k, op):
    it, npc = _iters(engine, _mesh(name, k), op, fa.PRECOND_AMG, numpy_count=True)
    jac, _ = _iters(engine, _mesh(name, k), op, fa.PRECOND_JACOBI)
    print(name, "amg", it, "numpy", npc, "jacobi", jac)
    assert abs(it - npc) <= 2 and it <= 40 and it < jac


@pytest.mark.gpu
def test_sphere_mesh(engine):
    it, npc = _iters(engine, _sphere(), "elastic", fa.PRECOND_AMG, clamp_width=0.1)
    assert it <= 40
    # the Tet20 sphere coarsens; its count, 49 in the NumPy restatement (the CPU count of _np_count on this matrix), is above the goal
    # of 40 that the Tet4 and Hex8 boxes meet
    m = _mesh("sphere20", 0)
    it, npc = _iters(engine, m, "elastic", fa.PRECOND_AMG, clamp_width=0.1, numpy_count=True)
    jac, _ = _iters(engine, m, "elastic", fa.PRECOND_JACOBI, clamp_width=0.1)
    print("sphere20 amg", it, "numpy", npc, "jacobi", jac)
    assert abs(it - npc) <= 2 and it <= 49 + 2 and it < jac


@pytest.mark.gpu
def test_free_floating_near_nullspace(engine):
    """no Dirichlet nodes, rigid-body modes: A_c B_c ~ 0 on every level (the device's A_c and B_c)"""
    m = _mesh("hex8", 12)
    asm, csr, _, s = _system(engine, m, "elastic", clamp=False)
    amg = fa.SmoothedAggregationAMG(asm, csr, near_nullspace="rigid_body")
    assert amg.num_levels >= 2
    for l in range(amg.num_levels):
        A, B = amg.level_matrix(l, "A"), amg.level_matrix(l, "B").toarray()
        assert np.linalg.norm(A @ B) <= 1e-10 * sp.linalg.norm(A) * np.linalg.norm(B), l
    amg.close()


@pytest.mark.gpu
def test_conjugate_gradient_with_amg(engine):
    import torch

    m = _mesh("tet4", 12)
    asm, csr, clamp, s = _system(engine, m, "elastic")
    amg = fa.SmoothedAggregationAMG(asm, csr)
    b = torch.ones(s * m.num_nodes(), dtype=torch.float64, device="cuda")
    x = torch.zeros_like(b)
    it = (fa.ConjugateGradient().with_operator(csr, asm).with_preconditioner(amg)
          .with_stopping_criterion(fa.RelativeResidualCriterion(1e-8)).solve_with_guess(b, x))
    x2 = torch.zeros_like(b)
    it2 = engine.cg_solve(csr.values, b, x2, fa.PRECOND_AMG, 1e-8)
    assert it == it2 and torch.equal(x, x2) and it < 40
    amg.close()


@pytest.mark.gpu
def test_numeric_refresh_matches_fresh_create(engine):
    import torch

    m = _mesh("hex8", 12)
    rng = np.random.default_rng(2)
    s = 3
    u1 = 0.01 * rng.standard_normal(s * m.num_nodes())
    u2 = u1 + 0.01 * rng.standard_normal(s * m.num_nodes())
    asm, csr1, clamp, _ = _system(engine, m, "neo_hookean", u=u1)
    amg = fa.SmoothedAggregationAMG(asm, csr1)
    engine2 = fa.Engine(0)
    asm2, csr2, _, _ = _system(engine2, m, "neo_hookean", u=u2)
    assert np.array_equal(csr1.row_offsets, csr2.row_offsets) and np.array_equal(csr1.col_indices, csr2.col_indices)
    amg.update(csr2)
    fresh = fa.SmoothedAggregationAMG(asm2, csr2)
    assert amg.num_levels == fresh.num_levels
    for l in range(amg.num_levels - 1):   # (theta = 0 and a nonzero pattern: the aggregates follow the pattern)
        assert np.array_equal(amg.aggregates(l), fresh.aggregates(l)), l
    for l in range(amg.num_levels):
        assert np.array_equal(amg.level_matrix(l, "A").data, fresh.level_matrix(l, "A").data)
        if l + 1 < amg.num_levels:
            assert np.array_equal(amg.level_matrix(l, "P").data, fresh.level_matrix(l, "P").data)
    r = torch.from_numpy(rng.standard_normal(s * m.num_nodes())).cuda()
    z1, z2 = torch.zeros_like(r), torch.zeros_like(r)
    amg.apply(r, z1)
    fresh.apply(r, z2)
    assert torch.equal(z1, z2)
    fresh.close()
    amg.close()
    engine2.close()


@pytest.mark.gpu
def test_error_contract(engine):
    import ctypes as C

    lib = _ffi.lib()
    m = _mesh("quad4", 8)
    asm, csr, clamp, s = _system(engine, m, "elastic")
    vp = C.c_void_p(csr.values.data_ptr())
    h = C.c_void_p()
    # FH_PRECOND_AMG without a hierarchy
    import torch

    n = s * m.num_nodes()
    b = torch.ones(n, dtype=torch.float64, device="cuda")
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    with pytest.raises(_ffi.FenrisError) as e:
        engine.cg_solve(csr.values, b, x, fa.PRECOND_AMG, 1e-8)
    assert e.value.code == FH_INVALID_STATE
    assert lib.fh_amg_create(engine._h, vp, _ffi.AMG_USER, None, 3, 0.0, 0, C.byref(h)) == FH_BAD_ARGUMENT
    Bu = np.ones((n, 7))
    assert lib.fh_amg_create(engine._h, vp, _ffi.AMG_USER, _ffi.fp(Bu), 7, 0.0, 0, C.byref(h)) == FH_BAD_ARGUMENT
    assert lib.fh_amg_create(engine._h, vp, _ffi.AMG_USER, _ffi.fp(Bu), 0, 0.0, 0, C.byref(h)) == FH_BAD_ARGUMENT
    # rigid-body modes need s = d
    e2 = fa.Engine(0)
    asm2, csr2, _, _ = _system(e2, _mesh("quad4", 8), "laplace")
    assert lib.fh_amg_create(e2._h, C.c_void_p(csr2.values.data_ptr()), _ffi.AMG_RIGID_BODY, None, 0, 0.0, 0, C.byref(h)) == FH_BAD_ARGUMENT
    e2.close()
    # no pattern
    fresh = fa.Engine(0)
    assert lib.fh_amg_create(fresh._h, vp, _ffi.AMG_CONSTANT, None, 0, 0.0, 0, C.byref(h)) == FH_INVALID_STATE
    fresh.close()
    # a coarsest level above 4096 dofs
    big = _mesh("hex8", 12)
    e3 = fa.Engine(0)
    asm3, csr3, _, _ = _system(e3, big, "elastic")
    assert lib.fh_amg_create(e3._h, C.c_void_p(csr3.values.data_ptr()), _ffi.AMG_RIGID_BODY, None, 0, 0.0, 1, C.byref(h)) == FH_UNSUPPORTED
    e3.close()
    # orphaning: destroying the context first
    e4 = fa.Engine(0)
    asm4, csr4, _, _ = _system(e4, _mesh("quad4", 8), "elastic")
    amg = fa.SmoothedAggregationAMG(asm4, csr4)
    e4.close()
    r = torch.zeros(n, dtype=torch.float64, device="cuda")
    assert lib.fh_amg_apply_dev(amg._h, C.c_void_p(r.data_ptr()), C.c_void_p(x.data_ptr())) == FH_BAD_ARGUMENT
    amg.close()
    # a small system: one level, the dense solve is exact
    amg = fa.SmoothedAggregationAMG(asm, csr)
    assert amg.num_levels == 1
    it = engine.cg_solve(csr.values, b, x, fa.PRECOND_AMG, 1e-10)
    assert it <= 2
    amg.close()
    # the matrix-free solves keep rejecting FH_PRECOND_AMG
    with pytest.raises(_ffi.FenrisError) as e:
        engine.cg_solve_matrix_free(b, x, fa.PRECOND_AMG, 1e-8)
    assert e.value.code == FH_BAD_ARGUMENT
