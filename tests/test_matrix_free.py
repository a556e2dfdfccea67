"""Matrix-free operator (fh_apply_operator_dev, fh_operator_diagonal_dev, fh_set_operator_dirichlet_nodes) and the PCG on it
(fh_cg_solve_matrix_free): y = A x against fh_spmv_dev on the matrix the CSR path assembles, |y_mf - y_ref|_inf <= 1e-12 | |K| |x| |_inf."""
import json
import os

import numpy as np
import pytest

import fenris_amd as fa
from fenris_amd import _ffi, quadrature
from conftest import GOLDEN

LAME = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.3))


@pytest.fixture()
def engine():
    eng = fa.Engine(0)   # one context per test: Dirichlet nodes and masks do not leak
    yield eng
    eng.close()


def _mesh(kind, res=3, seed=0, perturb=0.0):
    box3 = fa.procedural.create_unit_box_uniform_hex_mesh_3d
    tet3 = fa.procedural.create_unit_box_uniform_tet_mesh_3d
    quad2 = fa.procedural.create_unit_square_uniform_quad_mesh_2d
    tri2 = fa.procedural.create_unit_square_uniform_tri_mesh_2d
    make = {
        "QUAD4": (lambda: quad2(res), quadrature.tensor.quadrilateral_gauss(2)),
        "QUAD9": (lambda: fa.quad9_mesh_from_quad4(quad2(res)), quadrature.tensor.quadrilateral_gauss(3)),
        "TRI3": (lambda: tri2(res), quadrature.total_order.triangle(1)),
        "TRI6": (lambda: fa.tri6_mesh_from_tri3(tri2(res)), quadrature.total_order.triangle(2)),
        "HEX8": (lambda: box3(res), quadrature.tensor.hexahedron_gauss(2)),
        "HEX20": (lambda: fa.hex20_mesh_from_hex8(box3(2)), quadrature.tensor.hexahedron_gauss(3)),
        "HEX27": (lambda: fa.hex27_mesh_from_hex8(box3(2)), quadrature.tensor.hexahedron_gauss(3)),
        "TET4": (lambda: tet3(res), quadrature.total_order.tetrahedron(1)),
        "TET10": (lambda: fa.tet10_mesh_from_tet4(tet3(2)), quadrature.total_order.tetrahedron(2)),
        "TET20": (lambda: fa.tet20_mesh_from_tet4(tet3(1)), quadrature.total_order.tetrahedron(4)),
    }
    gen, (w, p) = make[kind]
    m = gen()
    if perturb:
        rng = np.random.default_rng(seed)
        m = fa.Mesh(m.vertices + perturb * rng.uniform(-1, 1, m.vertices.shape), m.connectivity, m.elem_kind)
    return m, np.asarray(w), np.asarray(p)


def _assembler(engine, m, op, qt):
    s = 1 if op == "laplace" else m.vertices.shape[1]
    opr = fa.LaplaceOperator() if op == "laplace" else fa.MaterialEllipticOperator(fa.LinearElasticMaterial())
    return (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(m).with_operator(opr)
            .with_quadrature_table(qt).with_u(np.zeros(s * m.num_nodes())).build())


def _uniform(op, w, p):
    qt = fa.UniformQuadratureTable.from_points_and_weights(p, w)
    return qt if op == "laplace" else qt.with_uniform_data(LAME)


def _check_against_spmv(engine, asm, rng, dirichlet=None):
    """operator vs fh_spmv_dev on the assembled (and, with Dirichlet nodes, modified) K"""
    import torch

    k = fa.CsrAssembler(fa.SCATTER_GATHER).assemble(asm, device_values=True)
    s = asm.solution_dim()
    if dirichlet is not None:
        fa.apply_homogeneous_dirichlet_bc_csr(k, dirichlet, s, asm)
    n = s * asm.engine.num_nodes()
    x = torch.from_numpy(rng.standard_normal(n)).cuda()
    y_ref = torch.zeros(n, dtype=torch.float64, device="cuda")
    engine.spmv(k.values, x, y_ref)
    op = fa.MatrixFreeOperator(asm)
    if dirichlet is not None:
        op.with_dirichlet_nodes(dirichlet)
    y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")   # overwritten: no NaN survives
    op.apply(y, x)
    ks = fa.CsrMatrix(k.row_offsets, k.col_indices, k.values.cpu().numpy()).to_scipy()
    bound = np.abs(abs(ks) @ np.abs(x.cpu().numpy())).max()
    err = np.abs(y.cpu().numpy() - y_ref.cpu().numpy()).max()
    assert np.isfinite(err) and err <= 1e-12 * bound, (err, bound)
    return op, k, ks


KINDS = ["QUAD4", "TRI3", "HEX8", "TET4", "QUAD9", "TRI6", "HEX20", "HEX27", "TET10", "TET20"]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("op", ["laplace", "elastic"])
def test_operator_matches_spmv_on_every_kind(engine, kind, op):
    rng = np.random.default_rng(KINDS.index(kind))
    m, w, p = _mesh(kind, perturb=0.02 if kind in ("HEX8", "QUAD4") else 0.0, seed=3)
    _check_against_spmv(engine, _assembler(engine, m, op, _uniform(op, w, p)), rng)


@pytest.mark.gpu
@pytest.mark.parametrize("perturb", [0.0, 0.03])   # all-affine box (moment form) and general hexahedra (point loop)
def test_operator_hex8_box_and_perturbed(engine, perturb):
    m, w, p = _mesh("HEX8", res=6, perturb=perturb, seed=5)
    for op in ("laplace", "elastic"):
        _check_against_spmv(engine, _assembler(engine, m, op, _uniform(op, w, p)), np.random.default_rng(7))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["HEX8", "TET4", "HEX27", "TRI6"])
@pytest.mark.parametrize("table", ["per_point", "compact", "rule_set"])
def test_operator_tables(engine, kind, table):
    rng = np.random.default_rng(11)
    m, w, p = _mesh(kind, perturb=0.0)
    nq = len(w)
    if table == "per_point":
        qt = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_data(
            [fa.LameParameters(1e5 * (1 + q), 2e5 * (2 + q % 3)) for q in range(nq)])
    else:
        emap = (np.arange(m.num_elements()) % 3 == 0).astype(np.uint64)
        if table == "compact":
            rules = [(w, p, [fa.LameParameters(1e5 * (r + 1), 3e5 + q) for q in range(nq)]) for r in range(2)]
        else:   # two point sets: the element kind's rule and a richer one
            if kind in ("HEX8", "HEX27"):
                w2, p2 = quadrature.tensor.hexahedron_gauss(4)
            elif kind == "TET4":
                w2, p2 = quadrature.total_order.tetrahedron(3)
            else:
                w2, p2 = quadrature.total_order.triangle(4)
            w2, p2 = np.asarray(w2), np.asarray(p2)
            rules = [(w, p, [LAME] * nq), (w2, p2, [fa.LameParameters(2e5, 7e5)] * len(w2))]
        qt = fa.compact_quadrature_table([r[1] for r in rules], [r[0] for r in rules], [r[2] for r in rules], emap)
    op, _, ks = _check_against_spmv(engine, _assembler(engine, m, "elastic", qt), rng)
    d_ref = ks.diagonal()   # the per-element parameters / the rule-set walk of the diagonal
    assert np.abs(op.diagonal() - d_ref).max() <= 1e-12 * np.abs(d_ref).max()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["HEX8", "TET4", "HEX27"])
def test_operator_under_element_mask_and_dirichlet(engine, kind):
    rng = np.random.default_rng(21)
    m, w, p = _mesh(kind)
    asm = _assembler(engine, m, "elastic", _uniform("elastic", w, p))
    engine.set_active_elements(rng.random(m.num_elements()) < 0.6)
    try:
        op, _, ks = _check_against_spmv(engine, asm, rng)
        d_ref = ks.diagonal()   # the masked diagonal (rows of nodes without an active element are zero)
        assert np.abs(op.diagonal() - d_ref).max() <= 1e-12 * np.abs(d_ref).max()
    finally:
        engine.set_active_elements(None)
    bc = np.where(m.vertices[:, 0] < 1e-9)[0]
    op, k, ks = _check_against_spmv(engine, asm, rng, dirichlet=bc)
    # the diagonal, with and without Dirichlet nodes
    d_ref = ks.diagonal()
    d = op.diagonal()
    assert np.abs(d - d_ref).max() <= 1e-12 * np.abs(d_ref).max()
    op.with_dirichlet_nodes(None)
    d0 = op.diagonal()
    d0_ref = fa.CsrAssembler(fa.SCATTER_GATHER).assemble(asm).to_scipy().diagonal()
    assert np.abs(d0 - d0_ref).max() <= 1e-12 * np.abs(d0_ref).max()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_diagonal_matches_assembled(engine, kind):
    m, w, p = _mesh(kind, perturb=0.02 if kind in ("HEX8", "TET4") else 0.0, seed=2)
    for op in ("laplace", "elastic"):
        asm = _assembler(engine, m, op, _uniform(op, w, p))
        d_ref = fa.CsrAssembler(fa.SCATTER_GATHER).assemble(asm).to_scipy().diagonal()
        d = fa.MatrixFreeOperator(asm).diagonal()
        assert np.abs(d - d_ref).max() <= 1e-12 * np.abs(d_ref).max(), (kind, op)


@pytest.mark.gpu
def test_operator_64_cubed_elasticity_with_dirichlet(engine):
    m = fa.procedural.create_unit_box_uniform_hex_mesh_3d(64)
    w, p = quadrature.tensor.hexahedron_gauss(2)
    asm = _assembler(engine, m, "elastic", _uniform("elastic", np.asarray(w), np.asarray(p)))
    bc = np.where(m.vertices[:, 2] < 1e-9)[0]
    _check_against_spmv(engine, asm, np.random.default_rng(64), dirichlet=bc)


@pytest.mark.gpu
def test_operator_contract(engine):
    import torch

    m, w, p = _mesh("HEX8", res=4, perturb=0.02, seed=1)
    asm = _assembler(engine, m, "elastic", _uniform("elastic", w, p))
    n = 3 * m.num_nodes()
    u = 0.01 * np.random.default_rng(2).standard_normal(n)
    asm.engine.set_u(u)
    r0 = fa.VectorAssembler().assemble_vector(asm)
    op = fa.MatrixFreeOperator(asm).with_dirichlet_nodes([0, 5, 9])
    x = torch.from_numpy(np.random.default_rng(3).standard_normal(n)).cuda()
    y1 = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    y2 = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    op.apply(y1, x)
    op.apply(y2, x)
    assert torch.isfinite(y1).all() and torch.equal(y1, y2)        # overwritten, bit for bit the same twice
    r1 = fa.VectorAssembler().assemble_vector(asm)
    assert np.array_equal(r0, r1)                                    # the context's u is neither read nor changed
    ynp = np.full(n, np.nan)
    op.apply(ynp, x.cpu().numpy())                                    # host arrays
    assert np.array_equal(ynp, y1.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("material", ["neo", "stvk", "mass", "tensor"])
def test_other_operators_are_unsupported(engine, material):
    import torch

    m, w, p = _mesh("HEX8", res=2)
    n = 3 * m.num_nodes()
    qt = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(LAME)
    opr = {"neo": lambda: fa.MaterialEllipticOperator(fa.NeoHookeanMaterial()),
           "stvk": lambda: fa.MaterialEllipticOperator(fa.StVKMaterial())}
    if material in opr:
        _assembler(engine, m, "elastic", qt)
        asm = (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(m).with_operator(opr[material]())
               .with_quadrature_table(qt).with_u(np.zeros(n)).build())
        eng = asm.engine
    else:
        eng = engine
        eng.set_mesh(m)
        eng.set_operator(_ffi.MASS_VECTOR if material == "mass" else _ffi.TENSOR)
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    with pytest.raises(fa.FenrisError) as exc:
        eng.apply_operator_dev(x, x.clone())
    assert exc.value.code == _ffi.FH_UNSUPPORTED
    with pytest.raises(fa.FenrisError) as exc:
        eng.operator_diagonal_dev(x)
    assert exc.value.code == _ffi.FH_UNSUPPORTED


@pytest.mark.gpu
def test_missing_mesh_or_table_is_invalid_state():
    import torch

    e = fa.Engine(0)
    try:
        x = torch.zeros(8, dtype=torch.float64, device="cuda")
        with pytest.raises(fa.FenrisError) as exc:
            e.apply_operator_dev(x, x.clone())
        assert exc.value.code == _ffi.FH_INVALID_STATE
        m, _, _ = _mesh("HEX8", res=1)
        e.set_mesh(m)
        e.set_operator(_ffi.LAPLACE)
        with pytest.raises(fa.FenrisError) as exc:
            e.apply_operator_dev(x, x.clone())
        assert exc.value.code == _ffi.FH_INVALID_STATE
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["HEX8", "HEX27"])
def test_collapsed_element_raises(engine, kind):
    import torch

    m, w, p = _mesh(kind, res=2)
    v = m.vertices.copy()
    v[np.asarray(m.connectivity[1]).astype(int)] = 0.0
    m = fa.Mesh(v, m.connectivity, m.elem_kind)
    asm = _assembler(engine, m, "laplace", _uniform("laplace", w, p))
    x = torch.ones(m.num_nodes(), dtype=torch.float64, device="cuda")
    with pytest.raises(fa.SingularJacobianError):
        fa.MatrixFreeOperator(asm).apply(x.clone(), x)
    with pytest.raises(fa.SingularJacobianError):
        fa.MatrixFreeOperator(asm).diagonal()


def _cantilever(engine, nx=16, ny=4, nz=4):
    m = fa.procedural.create_rectangular_uniform_hex_mesh(1.0, nx, ny, nz, 1)
    w, p = quadrature.tensor.hexahedron_gauss(2)
    asm = _assembler(engine, m, "elastic", _uniform("elastic", np.asarray(w), np.asarray(p)))
    bc = np.where(m.vertices[:, 0] < 1e-9)[0]
    return m, asm, bc


@pytest.mark.gpu
@pytest.mark.parametrize("pre", ["identity", "jacobi"])
def test_pcg_matches_assembled_pcg(engine, pre):
    import torch

    m, asm, bc = _cantilever(engine)
    n = 3 * m.num_nodes()
    b = torch.zeros(n, dtype=torch.float64, device="cuda")
    b[2::3] = -1.0 / m.num_nodes()
    fa.apply_homogeneous_dirichlet_bc_rhs(b, bc, 3)
    P = fa.JacobiPreconditioner() if pre == "jacobi" else fa.IdentityOperator()
    k = fa.CsrAssembler(fa.SCATTER_GATHER).assemble(asm, device_values=True)
    fa.apply_homogeneous_dirichlet_bc_csr(k, bc, 3, asm)

    def solve(operator, *extra):
        x = torch.zeros(n, dtype=torch.float64, device="cuda")
        it = (fa.ConjugateGradient.new().with_operator(operator, *extra).with_preconditioner(P).with_max_iter(20000)
              .with_stopping_criterion(fa.RelativeResidualCriterion(1e-9)).solve_with_guess(b, x))
        return x, it

    x_a, it_a = solve(k, asm)
    op = fa.MatrixFreeOperator(asm).with_dirichlet_nodes(bc)
    x_m, it_m = solve(op)
    x_m2, it_m2 = solve(op)
    assert torch.equal(x_m, x_m2) and it_m == it_m2
    assert (x_m - x_a).abs().max().item() <= 1e-7 * x_a.abs().max().item()
    assert abs(it_m - it_a) <= max(2, 0.02 * it_a), (it_m, it_a)
    # the host-array twin
    xh = np.zeros(n)
    it_h = asm.engine.cg_solve_matrix_free(b.cpu().numpy(), xh, 1 if pre == "jacobi" else 0, 1e-9, 20000)
    assert it_h == it_m and np.array_equal(xh, x_m.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind,nres", [("poisson2d_mms_quad4_summary", "QUAD4", 5),
                                            ("poisson3d_mms_hex8_summary", "HEX8", 4),
                                            ("poisson3d_mms_tet4_summary", "TET4", 3),
                                            ("poisson3d_mms_hex27_summary", "HEX27", 3),
                                            ("poisson2d_mms_tri3_summary", "TRI3", 5)])
def test_mms_loop_matrix_free(name, kind, nres):
    """test_solver.py's MMS loop with MatrixFreeOperator + Jacobi instead of an assembled K: the reference's errors at 1 %"""
    import torch

    ref = json.load(open(os.path.join(GOLDEN, "mms_reference_values.json")))["summaries"][name]
    if kind == "QUAD4":
        gen, rule, err_rule = (fa.procedural.create_unit_square_uniform_quad_mesh_2d, quadrature.tensor.quadrilateral_gauss(2),
                               quadrature.tensor.quadrilateral_gauss(6))
    elif kind == "HEX8":
        gen, rule, err_rule = (fa.procedural.create_unit_box_uniform_hex_mesh_3d, quadrature.tensor.hexahedron_gauss(2),
                               quadrature.tensor.hexahedron_gauss(6))
    elif kind == "HEX27":
        gen = lambda r: fa.hex27_mesh_from_hex8(fa.procedural.create_unit_box_uniform_hex_mesh_3d(r))
        rule, err_rule = quadrature.tensor.hexahedron_gauss(4), quadrature.tensor.hexahedron_gauss(6)
    elif kind == "TRI3":
        gen, rule, err_rule = (fa.procedural.create_unit_square_uniform_tri_mesh_2d, quadrature.total_order.triangle(0),
                               quadrature.total_order.triangle(6))
    else:
        t = json.load(open(os.path.join(GOLDEN, "tet_rule_6_24.json")))
        gen, rule, err_rule = (fa.procedural.create_unit_box_uniform_tet_mesh_3d, quadrature.total_order.tetrahedron(0),
                               (np.array(t["weights"]), np.array(t["points"])))

    def u_exact(x):
        return np.prod(np.sin(np.pi * x), axis=-1)[..., None]

    def u_grad(x):
        d = x.shape[-1]
        g = np.zeros(x.shape[:-1] + (d, 1))
        for i in range(d):
            t = np.pi * np.cos(np.pi * x[..., i])
            for j in range(d):
                if j != i:
                    t = t * np.sin(np.pi * x[..., j])
            g[..., i, 0] = t
        return g

    e_k, e_b, e_err = fa.Engine(0), fa.Engine(0), fa.Engine(0)
    try:
        for i, res in enumerate([1, 2, 4, 8, 16][:nres]):
            mesh = gen(res)
            w, p = rule
            d, N = mesh.vertices.shape[1], mesh.num_nodes()
            qt = fa.UniformQuadratureTable.from_points_and_weights(p, w)
            lap = (fa.ElementEllipticAssemblerBuilder(e_k).with_finite_element_space(mesh).with_operator(fa.LaplaceOperator())
                   .with_quadrature_table(qt).with_u(np.zeros(N)).build())
            src = (fa.ElementSourceAssemblerBuilder.new(e_b).with_finite_element_space(mesh)
                   .with_source(fa.SourceFunction(1, lambda x, _d: d * np.pi ** 2 * u_exact(x))).with_quadrature_table(qt).build())
            b = torch.zeros(N, dtype=torch.float64, device="cuda:0")
            fa.VectorAssembler().assemble_vector_into(b, src)
            bc = np.where(np.abs(mesh.vertices - 0.5).max(axis=1) > 0.4999)[0]
            fa.apply_homogeneous_dirichlet_bc_rhs(b, bc, 1)
            op = fa.MatrixFreeOperator(lap).with_dirichlet_nodes(bc)
            u_h = torch.zeros(N, dtype=torch.float64, device="cuda:0")
            (fa.ConjugateGradient.new().with_operator(op).with_preconditioner(fa.JacobiPreconditioner()).with_max_iter(10000)
             .with_stopping_criterion(fa.RelativeResidualCriterion(1e-9)).solve_with_guess(b, u_h))
            we, pe = err_rule
            err_asm = (fa.ElementSourceAssemblerBuilder.new(e_err).with_finite_element_space(mesh)
                       .with_source(fa.SourceFunction(1, lambda x, _d: u_exact(x)))
                       .with_quadrature_table(fa.UniformQuadratureTable.from_points_and_weights(pe, we)).build())
            uh = u_h.cpu().numpy()
            l2 = fa.estimate_L2_error(err_asm, u_exact, uh)
            h1 = fa.estimate_H1_seminorm_error(err_asm, u_grad, uh)
            assert abs(l2 - ref["L2_errors"][i]) / ref["L2_errors"][i] < 0.01, (res, l2, ref["L2_errors"][i])
            assert abs(h1 - ref["H1_seminorm_errors"][i]) / ref["H1_seminorm_errors"][i] < 0.01, (res, h1)
    finally:
        e_k.close(), e_b.close(), e_err.close()


def test_matrix_free_entry_points_are_declared():
    """no GPU: the new entry points are in the header and the ctypes table"""
    hdr = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "fenris_hip.h")).read()
    for name in ("fh_set_operator_dirichlet_nodes", "fh_apply_operator_dev", "fh_operator_diagonal_dev", "fh_cg_solve_matrix_free",
                 "fh_cg_solve_matrix_free_dev"):
        assert name + "(" in hdr and name in _ffi.exported_symbols()
    assert hasattr(fa, "MatrixFreeOperator")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["HEX27", "TET10"])
def test_outside_the_tiles_applies_and_solves_are_bitwise_reproducible(engine, kind):
    """the kinds outside the tiles take k_mf_apply_elements + the ordered node sums: no atomics, the same bits every run"""
    import torch

    m, w, p = _mesh(kind)
    asm = _assembler(engine, m, "elastic", _uniform("elastic", w, p))
    bc = np.where(m.vertices[:, 0] < 1e-9)[0]
    op = fa.MatrixFreeOperator(asm).with_dirichlet_nodes(bc)
    n = 3 * m.num_nodes()
    x = torch.from_numpy(np.random.default_rng(4).standard_normal(n)).cuda()
    ys = []
    for _ in range(3):
        y = torch.empty_like(x)
        op.apply(y, x)
        ys.append(y)
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])
    b = torch.zeros(n, dtype=torch.float64, device="cuda")
    b[2::3] = -1.0
    fa.apply_homogeneous_dirichlet_bc_rhs(b, bc, 3)
    sols = []
    for _ in range(2):
        u = torch.zeros(n, dtype=torch.float64, device="cuda")
        it = (fa.ConjugateGradient.new().with_operator(op).with_preconditioner(fa.JacobiPreconditioner()).with_max_iter(5000)
              .with_stopping_criterion(fa.RelativeResidualCriterion(1e-9)).solve_with_guess(b, u))
        sols.append((u, it))
    assert sols[0][1] == sols[1][1] and torch.equal(sols[0][0], sols[1][0])


@pytest.mark.gpu
def test_operators_sharing_an_assembler_keep_their_own_nodes(engine):
    import torch

    m, w, p = _mesh("HEX8", res=3)
    asm = _assembler(engine, m, "elastic", _uniform("elastic", w, p))
    n = 3 * m.num_nodes()
    x = torch.from_numpy(np.random.default_rng(5).standard_normal(n)).cuda()
    fixed = fa.MatrixFreeOperator(asm).with_dirichlet_nodes(np.where(m.vertices[:, 0] < 1e-9)[0])
    y1 = torch.empty_like(x)
    fixed.apply(y1, x)
    free = fa.MatrixFreeOperator(asm)
    y_free = torch.empty_like(x)
    free.apply(y_free, x)
    y2 = torch.empty_like(x)
    fixed.apply(y2, x)
    assert torch.equal(y1, y2) and not torch.equal(y1, y_free)


@pytest.mark.gpu
def test_large_constrained_entries_do_not_cost_the_free_rows_precision(engine):
    """the operand's scale comes from the entries the element pass sees: x with constrained entries 1e15 times the free ones"""
    import torch

    m, w, p = _mesh("HEX8", res=4)
    asm = _assembler(engine, m, "elastic", _uniform("elastic", w, p))
    bc = np.where(m.vertices[:, 0] < 1e-9)[0]
    k = fa.CsrAssembler(fa.SCATTER_GATHER).assemble(asm, device_values=True)
    fa.apply_homogeneous_dirichlet_bc_csr(k, bc, 3, asm)
    n = 3 * m.num_nodes()
    rng = np.random.default_rng(6)
    xh = 1e-9 * rng.standard_normal(n)
    cons = np.zeros(n, dtype=bool)
    for c in range(3):
        cons[3 * bc + c] = True
    xh[cons] = 1e6 * rng.standard_normal(cons.sum())
    x = torch.from_numpy(xh).cuda()
    y_ref = torch.zeros(n, dtype=torch.float64, device="cuda")
    engine.spmv(k.values, x, y_ref)
    y = torch.empty_like(x)
    fa.MatrixFreeOperator(asm).with_dirichlet_nodes(bc).apply(y, x)
    ks = fa.CsrMatrix(k.row_offsets, k.col_indices, k.values.cpu().numpy()).to_scipy()
    free = ~cons
    bound = (abs(ks) @ np.where(free, np.abs(xh), 0.0))[free].max()
    err = np.abs(y.cpu().numpy() - y_ref.cpu().numpy())[free].max()
    assert err <= 1e-12 * bound, (err, bound)
