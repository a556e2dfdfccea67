"""The linear kernels on stretched, sheared, graded, shifted, scaled and mirrored meshes (geometry_cases.py), entry by entry against the
long-double reference (hp_reference.py).

The bar, for every kernel alike:   |dev - ref| <= 1e-12 gamma scale,   entry by entry (matrices, diagonals) or row by row (maps, residuals).
`scale` is the assembled term scale T of hp_reference.Reference (the sum of the magnitudes of the terms an entry is made of: no
cancellation credited), for a map (T |x|)_i, for the mass the entry itself; gamma = 1 but on `shifted`, where the rounding of the
coordinates themselves enters J at eps |X| / h (geometry_cases.element_gamma, folded in per element).  A plain double evaluation of the
reference holds 1 / 64 of this bar on every case (test_geometry_cases.py).  The global bars of the other modules (1e-12 max |K|) see
nothing of the small entries of such meshes: on the 1 : 1 : 1e-4 plate they span ten decades.

Every assembly asserts the kernel that ran and the affine classification against the host's prediction; the largest error / bar per kernel
family and geometry is printed at the end of the module."""
import numpy as np
import pytest

import fenris_amd as fa
import geometry_cases as gc
import hp_reference as hp

pytestmark = pytest.mark.gpu
BAR = 1e-12
LAME = fa.LameParameters(3.0e2, 5.0e2)
RHO = 2.5
TWO_PASS_DENSE = "k_assemble_matrix<dump> + k_rows_from_dense"
TWO_PASS_TRI = "k_assemble_matrix<dump> + k_rows_from_tri"
HEX27_MFMA = "k_hex27_dense_blocks + k_rows_from_tri"
MIXED = "k_affine_rows + k_hex8_rows"
FAMILIES = {"k_affine_rows", "k_hex8_rows", MIXED, "k_gather_rows", "k_gather_pipelined", "k_assemble_matrix<gather>", TWO_PASS_DENSE,
            TWO_PASS_TRI, HEX27_MFMA, "k_assemble_matrix<atomic>", "k_assemble_matrix<colored>"}   # (atomic and colored: one family, the scatter modes)
SYMMETRIC_BITWISE = ("k_affine_rows", "k_hex8_rows")           # promised by test_affine.py and test_hex8_rows.py
SCATTER_GEOMETRIES = ("plate_1e4", "graded", "shifted")
MASS_GEOMETRIES = ("graded", "plate_1e4", "shifted", "mirrored")
MF_GEOMETRIES = ("plate_1e4", "needle_1e3", "shear", "graded", "shifted", "mirrored")
MF_MESHES = [("HEX8", "exact"), ("HEX8", "jittered"), ("TET4", "exact"), ("QUAD4", "jittered"), ("TRI3", "exact")]
OPERATOR_ROUTE = "k_element_pass_tiled + k_operator_from_partials"
DIAGONAL_ROUTE = "k_diagonal_tiled + k_vector_from_partials"
VECTOR_ROUTE = "k_element_pass_tiled + k_vector_from_partials"
MARGINS = {}


def _le(key, err, bar, detail=""):
    """|err| <= bar entry by entry; records the largest err / bar under the key"""
    err, bar = np.abs(np.asarray(err, dtype=np.longdouble)), np.asarray(bar, dtype=np.longdouble)
    assert np.all(np.isfinite(err.astype(np.float64))) and np.all(bar >= 0), key
    with np.errstate(divide="ignore", invalid="ignore"):           # (scale 0: every term of the entry is zero, and so must the entry be)
        ratio = np.where(err == 0, 0, err / bar).reshape(-1)
    worst = int(np.argmax(ratio))
    frac = float(ratio[worst])
    MARGINS[key] = max(MARGINS.get(key, 0.0), frac)
    print(f"{key} {detail}: largest error / bar {frac:.3e} (entry {worst}: error {float(err.reshape(-1)[worst]):.3e}, scale "
          f"{float(bar.reshape(-1)[worst]) / BAR:.3e})")
    assert frac <= 1.0, (key, detail, frac)


@pytest.fixture(scope="module", autouse=True)
def _print_margins():
    yield
    if MARGINS:
        print("\nlargest error / (1e-12 gamma scale) per kernel family and geometry:")
        for k in sorted(MARGINS):
            print(f"  {k:100s} {MARGINS[k]:.3e}")


@pytest.fixture()
def engine():
    eng = fa.Engine(0)
    yield eng
    eng.close()


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


_CASES, _REFS = {}, {}


def case(kind, variant, geometry):
    key = (kind, variant, geometry)
    if key not in _CASES:
        _CASES[key] = gc.case(kind, variant, geometry)
    return _CASES[key]


def reference(c, model, gauss=None):
    """the long-double reference of the case (u: the smooth field of the residual checks; K of the linear operators does not read it),
    built once and left unchanged"""
    key = (c.kind, c.variant, c.geometry, model, gauss)
    if key not in _REFS:
        w, p = gc.rule_of(c.kind, gauss)
        s = 1 if model == "LAPLACE" else c.mesh.vertices.shape[1]
        _REFS[key] = hp.Reference(c.kind, model, c.mesh.vertices, c.mesh.connectivity, w, p, gc.smooth_u(np.asarray(c.mesh.vertices), s),
                                  LAME.mu, LAME.lambda_, rho=RHO)
    return _REFS[key]


def _assembler(eng, c, model, gauss=None, u=None, per_point=False):
    w, p = gc.rule_of(c.kind, gauss)
    qt = fa.UniformQuadratureTable.from_points_and_weights(p, w)
    if model == "LAPLACE":
        op = fa.LaplaceOperator()
    else:
        op = fa.MaterialEllipticOperator({"LINEAR_ELASTIC": fa.LinearElasticMaterial, "NEO_HOOKEAN": fa.NeoHookeanMaterial}[model]())
        qt = qt.with_data([fa.LameParameters(LAME.mu, LAME.lambda_) for _ in w]) if per_point else qt.with_uniform_data(LAME)
    return fa.ElementEllipticAssemblerBuilder(eng).with_finite_element_space(c.mesh).with_operator(op).with_quadrature_table(qt).with_u(u).build()


# ---- the assembled matrices: (label, model of the device, model of the reference, rule, scatter mode, kernel, switches)
def routes(kind, variant, geometry):
    G, A, C = "SCATTER_GATHER", "SCATTER_ATOMIC", "SCATTER_COLORED"
    out = []
    if kind == "HEX8":
        gather = MIXED if geometry == "threshold" else "k_affine_rows" if variant == "exact" else "k_hex8_rows"
        out += [("LAPLACE", "LAPLACE", None, G, gather, ()), ("LINEAR_ELASTIC", "LINEAR_ELASTIC", None, G, gather, ())]
        if geometry == "threshold":
            return out
        if variant == "jittered":
            out.append(("LINEAR_ELASTIC", "LINEAR_ELASTIC", 3, G, "k_gather_pipelined", ()))
        # parameters handed over point by point, the same value at every point: the switch keeps the library from noticing
        out.append(("LINEAR_ELASTIC", "LINEAR_ELASTIC", None, G, "k_assemble_matrix<gather>", ("FENRIS_HIP_NO_FAST",)))
        out.append(("NEO_HOOKEAN", "LINEAR_ELASTIC", None, G, TWO_PASS_TRI, ()))
        if geometry in SCATTER_GEOMETRIES:
            out += [("LINEAR_ELASTIC", "LINEAR_ELASTIC", None, A, "k_assemble_matrix<atomic>", ()),
                    ("LINEAR_ELASTIC", "LINEAR_ELASTIC", None, C, "k_assemble_matrix<colored>", ())]
    elif kind == "TET4":
        out += [("LAPLACE", "LAPLACE", None, G, "k_gather_rows", ()), ("LINEAR_ELASTIC", "LINEAR_ELASTIC", None, G, "k_gather_rows", ()),
                ("NEO_HOOKEAN", "LINEAR_ELASTIC", None, G, TWO_PASS_TRI, ())]
    elif kind in ("QUAD4", "TRI3"):
        out += [("LAPLACE", "LAPLACE", None, G, "k_gather_pipelined", ()), ("LINEAR_ELASTIC", "LINEAR_ELASTIC", None, G, "k_gather_pipelined", ())]
    elif kind == "HEX27":
        out += [("LAPLACE", "LAPLACE", None, G, TWO_PASS_DENSE, ()), ("LINEAR_ELASTIC", "LINEAR_ELASTIC", None, G, HEX27_MFMA, ())]
    else:
        out.append(("LINEAR_ELASTIC", "LINEAR_ELASTIC", None, G, TWO_PASS_TRI, ()))
    return out


def test_the_routes_name_every_family():
    names = {r[4] for c in gc.all_cases() for r in routes(*c)}
    assert names == FAMILIES
    for g in SCATTER_GEOMETRIES:
        assert {"k_assemble_matrix<atomic>", "k_assemble_matrix<colored>"} <= {r[4] for v in gc.VARIANTS for r in routes("HEX8", v, g)}


ASSEMBLED = gc.all_cases()


@pytest.mark.parametrize("kind,variant,geometry", ASSEMBLED, ids=["-".join(c) for c in ASSEMBLED])
def test_assembled_matrix_entry_by_entry(kind, variant, geometry):
    c = case(kind, variant, geometry)
    gamma = gc.gamma_of(c)
    E = c.mesh.num_elements()
    for model, ref_model, gauss, scatter, kernel, switches in routes(kind, variant, geometry):
        ref = reference(c, ref_model, gauss)
        ro, ci = ref.pattern()
        want, T = ref.csr_values(ro, ci), ref.csr_term_scale(ro, ci, gamma=gamma)
        eng = fa.Engine(0)
        try:
            for sw in switches:
                eng.set_option(sw, 1)
            u = np.zeros(ref.ndof) if model == "NEO_HOOKEAN" else None
            asm = _assembler(eng, c, model, gauss, u, per_point=bool(switches))
            if scatter == "SCATTER_COLORED":
                eng.color()
            assembler = fa.CsrAssembler(getattr(fa, scatter))
            k = assembler.assemble(asm)
            name = eng.last_kernel_name()
            assert name == kernel, (name, kernel)
            if kind == "HEX8" and kernel in ("k_affine_rows", "k_hex8_rows", "k_gather_pipelined", MIXED):
                n_el, n_aff_blk, n_gen_blk = eng.affine_stats()
                assert n_el == gc.predicted_affine_elements(c), (n_el, E)
                assert (n_aff_blk > 0) == (n_el > 0) and (n_gen_blk > 0) == (n_el < E)
            assert np.array_equal(k.row_offsets, ro) and np.array_equal(k.col_indices, ci)
            key = f"K {kernel} | {kind} {variant} | {geometry}"
            detail = f"{model}" + (f" gauss {gauss}" if gauss else "")
            vals = _host(k.values).copy()
            _le(key, vals - want, BAR * T, detail)
            if kernel in SYMMETRIC_BITWISE:
                a = k.to_scipy()
                assert (a != a.T).nnz == 0, key
            assembler.assemble_into_csr(k, asm)                     # on top of the values: 2 K at twice the bar
            _le(key + " | accumulated", _host(k.values) - 2 * want, 2 * BAR * T, detail)
        finally:
            eng.close()


# ---- the mass matrix: a relative error per entry
MASS = [(k, v, g) for (k, v) in (("HEX8", "exact"), ("HEX8", "jittered"), ("TET4", "exact")) for g in MASS_GEOMETRIES]


@pytest.mark.parametrize("s", [1, 3])
@pytest.mark.parametrize("kind,variant,geometry", MASS, ids=["-".join(c) for c in MASS])
def test_mass_matrix_entry_by_entry(engine, kind, variant, geometry, s):
    c = case(kind, variant, geometry)
    ref = reference(c, "LAPLACE" if s == 1 else "LINEAR_ELASTIC")
    ro, ci = ref.pattern()
    qt = fa.UniformQuadratureTable.from_points_and_weights(c.p, c.w).with_data([fa.Density(RHO) for _ in c.w])
    asm = fa.ElementMassAssembler.with_solution_dim(s, engine).with_space(c.mesh).with_quadrature_table(qt)
    k = fa.CsrAssembler(fa.SCATTER_GATHER).assemble(asm)
    name = engine.last_kernel_name()
    assert name in FAMILIES, name
    assert np.array_equal(k.row_offsets, ro) and np.array_equal(k.col_indices, ci)
    want = ref.csr_values(ro, ci, "M")
    on = want != 0                                                  # (s = 3: the pattern holds the zeros between the components)
    vals = _host(k.values)
    assert not np.any(vals[~on])
    _le(f"M {name} | {kind} {variant} | {geometry}", (vals - want)[on], BAR * ref.csr_term_scale(ro, ci, "M", gamma=gc.gamma_of(c))[on], f"s = {s}")


# ---- the matrix-free routes, row by row
MATRIX_FREE = [(k, v, g) for (k, v) in MF_MESHES for g in MF_GEOMETRIES]


@pytest.mark.parametrize("model", ["LAPLACE", "LINEAR_ELASTIC"])
@pytest.mark.parametrize("kind,variant,geometry", MATRIX_FREE, ids=["-".join(c) for c in MATRIX_FREE])
def test_matrix_free_routes_row_by_row(engine, kind, variant, geometry, model):
    c = case(kind, variant, geometry)
    gamma = gc.gamma_of(c)
    ref = reference(c, model)
    s = ref.s
    u = gc.smooth_u(np.asarray(c.mesh.vertices), s)
    asm = _assembler(engine, c, model, u=u)
    tag = f"{kind} {variant} | {geometry}"
    x = np.random.default_rng(41).uniform(-1.0, 1.0, ref.ndof)
    # the map
    op = fa.MatrixFreeOperator(asm)
    y = np.full(ref.ndof, np.nan)
    op.apply(y, x)
    assert engine.last_kernel_name() == OPERATOR_ROUTE, engine.last_kernel_name()
    if kind == "HEX8":   # exact: the element pass takes J as constant without testing (every element affine); jittered: no element is
        assert engine.affine_stats()[0] == gc.predicted_affine_elements(c) == (c.mesh.num_elements() if variant == "exact" else 0)
    _le(f"apply {OPERATOR_ROUTE} | {tag}", y - ref.apply(x)[0], BAR * ref.abs_apply_terms(x, gamma=gamma), model)
    # its diagonal
    d = op.diagonal()
    assert engine.last_kernel_name() == DIAGONAL_ROUTE, engine.last_kernel_name()
    _le(f"diagonal {DIAGONAL_ROUTE} | {tag}", d - ref.diagonal(), BAR * ref.diagonal_term_scale(gamma=gamma), model)
    # the residual at a smooth u: r = K u
    r = fa.VectorAssembler().assemble_vector(asm)
    assert engine.last_kernel_name() == VECTOR_ROUTE, engine.last_kernel_name()
    _le(f"residual {VECTOR_ROUTE} | {tag}", r - ref.residual(), BAR * ref.abs_apply_terms(u, gamma=gamma), model)
    # alpha M + beta K with both terms of one size on the diagonal
    alpha = 1.0
    beta = float(ref.diagonal("M").max() / ref.diagonal().max())
    sh = fa.MatrixFreeShiftedTangent(asm, RHO, alpha, beta)
    y = np.full(ref.ndof, np.nan)
    sh.apply(y, x)
    name = engine.last_kernel_name()
    assert name == ("k_shifted_pass_tiled + k_operator_from_partials" if kind == "HEX8" else OPERATOR_ROUTE), name
    label = name if kind == "HEX8" else "k_element_pass_tiled + k_mass_tiled + k_shift_from_partials"
    _le(f"shifted apply {label} | {tag}", y - ref.apply(x, alpha, beta)[0], BAR * ref.abs_apply_terms(x, alpha, beta, gamma=gamma), model)
