"""The hyperelastic kernels far from F = I, against the long-double reference of tests/hp_reference.py.

Deformations (det F > 0 at every point, asserted from the reference):
  (a) u = A X with cond F ~ 10 (the stretch 3 x 1 x 1/3 with shear of test_hex27_mfma.py),
  (b) u = A X with cond F ~ 100 (stretch 10 x 1 x 0.1 with shear),
  (c) compression to det F = 0.05 of a nearly incompressible material (ln J = -3),
  (d) a bend of the box into a quarter arc: rotations up to 90 degrees, moderate stretch, F different at every point,
  (e) a rigid rotation by an exactly representable R (the 120 degree cyclic permutation about (1, 1, 1); 90 degrees in 2D).
Routes: the assembled K(u) (two-pass generic, Hex27 matrix cores with and without them, one-pass gather / atomic / coloured and a row range),
the matrix-free tangent and its diagonal (tiles, element pass), the shifted tangent alpha M + beta K(u), the residual and the energy.
Bars (no route loosened): K 1e-12 max|K|, apply 1e-12 || |K| |x| ||, diagonal 1e-12 max|d|, residual 1e-12 of its absolute scale, energy
1e-12 sum |psi_e|.  Under a rigid rotation r and psi vanish: their scales are then the magnitudes of the TERMS of P and psi (hp_reference).
Case (e) also checks the device against itself: K(u_R) = R K(0) R^T block by block, with no reference at all."""
import numpy as np
import pytest

import fenris_amd as fa
from fenris_amd import quadrature
import hp_reference as hp

BAR = 1e-12
LAME = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.3))
LAME_NI = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.45))   # case (c): nearly incompressible
RHO = 2.5e3
OPS = {"NEO_HOOKEAN": fa.NeoHookeanMaterial, "STVK": fa.StVKMaterial}
R3 = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])   # x -> z -> y -> x: 120 degrees about (1, 1, 1)
R2 = np.array([[0.0, -1.0], [1.0, 0.0]])
F3 = {"a": np.array([[3.0, 0.4, 0.0], [0.0, 1.0, 0.3], [0.2, 0.0, 1.0 / 3.0]]),
      "b": np.array([[10.0, 1.5, 0.0], [0.0, 1.0, 0.2], [0.3, 0.0, 0.1]]),
      "c": np.array([[0.5, 0.1, 0.0], [0.0, 0.4, 0.05], [0.0, 0.0, 0.25]]),
      "e": R3}
F2 = {"a": np.array([[3.0, 0.4], [0.2, 1.0 / 3.0]]), "b": np.array([[10.0, 0.5], [0.2, 0.1]]), "e": R2}
COND = {"a": (8, 12), "b": (80, 130)}


def deformation(case, X):
    """nodal u of the case at the vertices X (N, d)"""
    d = X.shape[1]
    if case == "d":   # x in [0, 1] goes round a quarter circle of radius R0; z across it (thickness 0.8), y stretched by 0.9
        R0 = 2.0 / np.pi
        th = 0.5 * np.pi * X[:, 0]
        r = R0 + 0.8 * (X[:, 2] - 0.5)
        x = np.stack([r * np.sin(th), 0.9 * X[:, 1], 0.5 - R0 + r * np.cos(th)], axis=1)
        return (x - X).reshape(-1)
    F = (F3 if d == 3 else F2)[case]
    return (X @ (F - np.eye(d)).T).reshape(-1)


def _perturbed(m, amp, seed):
    rng = np.random.default_rng(seed)
    return fa.Mesh(m.vertices + amp * rng.uniform(-1, 1, m.vertices.shape), m.connectivity, m.elem_kind)


def mesh_of(variant):
    """(kind, mesh, weights, points): the tiled kinds with more than 256 elements (several tiles, a ragged last one)"""
    hexbox = fa.procedural.create_rectangular_uniform_hex_mesh(1.0 / 9.0, 9, 7, 6, 1)   # 378 parallelepipeds in [0, 1] x [0, 7/9] x [0, 2/3]
    if variant == "HEX8_AFFINE":
        m, (w, p) = hexbox, quadrature.tensor.hexahedron_gauss(2)
    elif variant == "HEX8_GENERAL":
        m, (w, p) = _perturbed(hexbox, 0.01, 3), quadrature.tensor.hexahedron_gauss(2)
    elif variant == "TET4":
        m, (w, p) = fa.procedural.create_unit_box_uniform_tet_mesh_3d(4), quadrature.total_order.tetrahedron(2)   # 768
    elif variant == "QUAD4":
        m, (w, p) = _perturbed(fa.procedural.create_unit_square_uniform_quad_mesh_2d(20), 0.005, 4), quadrature.tensor.quadrilateral_gauss(2)
    elif variant == "TRI3":
        m, (w, p) = fa.procedural.create_unit_square_uniform_tri_mesh_2d(12), quadrature.total_order.triangle(2)   # 288
    elif variant == "TET10":
        m, (w, p) = fa.tet10_mesh_from_tet4(fa.procedural.create_unit_box_uniform_tet_mesh_3d(2)), quadrature.total_order.tetrahedron(2)
    elif variant == "HEX27":
        m8 = _perturbed(fa.procedural.create_rectangular_uniform_hex_mesh(0.5, 2, 2, 2, 1), 0.04, 13)
        m, (w, p) = fa.hex27_mesh_from_hex8(m8), quadrature.tensor.hexahedron_gauss(3)
    return variant.split("_")[0], m, np.asarray(w), np.asarray(p)


def lame_of(case):
    return LAME_NI if case == "c" else LAME


def reference(kind, model, m, w, p, u, case):
    lm = lame_of(case)
    ref = hp.Reference(kind, model, m.vertices, m.connectivity, w, p, u, lm.mu, lm.lambda_, rho=RHO)
    assert ref.det_F_min > 0.0
    return ref


# ------------------------------------------------------------------------------------------------------------------ CPU: the reference itself
def _small(kind, seed=0):
    """a few distorted elements of each kind on [0, 1]^d"""
    rng = np.random.default_rng(seed)
    if kind in ("HEX8", "HEX27"):
        m = fa.procedural.create_rectangular_uniform_hex_mesh(0.5, 2, 1, 2, 1)
        m = fa.Mesh(m.vertices + 0.03 * rng.uniform(-1, 1, m.vertices.shape), m.connectivity, m.elem_kind)
        if kind == "HEX27":
            return m8_to(kind, m), quadrature.tensor.hexahedron_gauss(3)
        return m, quadrature.tensor.hexahedron_gauss(2)
    if kind in ("TET4", "TET10"):
        m = fa.procedural.create_unit_box_uniform_tet_mesh_3d(1)
        m = fa.Mesh(m.vertices + 0.03 * rng.uniform(-1, 1, m.vertices.shape), m.connectivity, m.elem_kind)
        return (m8_to(kind, m), quadrature.total_order.tetrahedron(2)) if kind == "TET10" else (m, quadrature.total_order.tetrahedron(2))
    if kind == "QUAD4":
        m = fa.procedural.create_unit_square_uniform_quad_mesh_2d(2)
        return fa.Mesh(m.vertices + 0.03 * rng.uniform(-1, 1, m.vertices.shape), m.connectivity, m.elem_kind), quadrature.tensor.quadrilateral_gauss(2)
    m = fa.procedural.create_unit_square_uniform_tri_mesh_2d(2)
    return fa.Mesh(m.vertices + 0.03 * rng.uniform(-1, 1, m.vertices.shape), m.connectivity, m.elem_kind), quadrature.total_order.triangle(2)


def m8_to(kind, m):
    return fa.hex27_mesh_from_hex8(m) if kind == "HEX27" else fa.tet10_mesh_from_tet4(m)


KINDS = ["HEX8", "TET4", "QUAD4", "TRI3", "HEX27", "TET10"]
CPU_CASES = [(k, c) for k in KINDS for c in ("mild", "a", "b", "e") + (("c", "d") if k in ("HEX8", "TET4") else ())]


def _u(case, X, seed=0):
    if case == "mild":
        return 0.05 * np.random.default_rng(seed).standard_normal(X.size)
    return deformation(case, X)


@pytest.mark.parametrize("kind", KINDS)
def test_shape_functions_pin_the_oracle_node_order(oracle, kind):
    K = getattr(oracle, kind)
    n, d = hp.KINDS[kind]
    for xi in np.random.default_rng(1).uniform(-1.0, 0.4, (7, d)):
        phi, g = hp.shape(kind, xi)
        assert phi.dtype == np.longdouble and g.shape == (n, d)
        assert np.abs(oracle.element_gradients(K, xi).T - g.astype(np.float64)).max() <= 1e-15
        assert np.abs(oracle.element_basis(K, xi) - phi.astype(np.float64)).max() <= 1e-15


def test_det_and_inverse_by_cofactors_in_long_double():
    rng = np.random.default_rng(0)
    for d in (2, 3):
        A = rng.standard_normal((20, d, d)).astype(np.longdouble)
        B = hp.inv(A)
        err = np.abs(A @ B - np.eye(d, dtype=np.longdouble)).max()
        assert B.dtype == np.longdouble and err <= 1e-16
        assert np.abs(hp.det(A).astype(np.float64) - np.linalg.det(A.astype(np.float64))).max() <= 1e-14


@pytest.mark.parametrize("kind,case", CPU_CASES)
@pytest.mark.parametrize("model", ["NEO_HOOKEAN", "STVK"])
def test_reference_agrees_with_the_oracle(oracle, kind, case, model):
    m, (w, p) = _small(kind)
    w, p = np.asarray(w), np.asarray(p)
    u = _u(case, m.vertices, seed=len(kind))
    ref = reference(kind, model, m, w, p, u, case)
    lm = lame_of(case)
    orc = oracle.ElementAssembler(getattr(oracle, kind), getattr(oracle, model), m.vertices, m.connectivity, w, p, params=lm.as_pair(), u=u)
    st, _, ro, ci, vals = oracle.assemble(orc)
    assert st == 0
    k = ref.csr_values(ro, ci)
    assert np.abs(vals - k).max() <= 1e-13 * np.abs(k).max()
    assert np.abs(np.diagonal(ref_dense(ro, ci, vals)) - ref.diagonal()).max() <= 1e-13 * np.abs(ref.diagonal()).max()
    st, _, f = oracle.assemble_vector(orc)
    assert st == 0
    scale = ref.residual_scale(terms=(case == "e")).max()
    assert np.abs(f - ref.residual()).max() <= 1e-13 * scale
    res = oracle.assemble_scalar(orc)
    assert res[0] == 0 and abs(res[-1] - ref.energy()) <= 1e-13 * ref.energy_scale(terms=(case == "e"))
    if case in COND:   # the case is what it says
        lo, hi = COND[case]
        F = (F3 if m.vertices.shape[1] == 3 else F2)[case]
        assert lo <= np.linalg.cond(F) <= hi


def ref_dense(ro, ci, vals):
    n = len(ro) - 1
    A = np.zeros((n, n))
    for r in range(n):
        A[r, np.asarray(ci[ro[r]:ro[r + 1]]).astype(np.int64)] = vals[ro[r]:ro[r + 1]]
    return A


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("model", ["NEO_HOOKEAN", "STVK", "LINEAR_ELASTIC"])
def test_reference_derivatives_by_central_differences(kind, model):
    """K x = (r(u + h x) - r(u - h x)) / 2h and r . x = (E(u + h x) - E(u - h x)) / 2h, all in long double, at a large strain"""
    m, (w, p) = _small(kind, seed=2)
    w, p = np.asarray(w), np.asarray(p)
    u = deformation("a", m.vertices)
    ld = np.longdouble
    x = np.random.default_rng(3).standard_normal(u.size).astype(ld)
    h = ld(1e-7)

    def at(v):
        return hp.Reference(kind, model, m.vertices, m.connectivity, w, p, v, LAME.mu, LAME.lambda_)

    ref, rp, rm = at(u), at(u.astype(ld) + h * x), at(u.astype(ld) - h * x)
    kx = ref.apply(x)[0]
    fd = (rp.residual() - rm.residual()) / (2 * h)
    assert np.abs(fd - kx).max() <= 1e-9 * np.abs(kx).max(), float(np.abs(fd - kx).max() / np.abs(kx).max())
    rx = np.dot(ref.residual(), x)
    fe = (rp.energy() - rm.energy()) / (2 * h)
    assert abs(fe - rx) <= 1e-9 * np.dot(ref.residual_scale(), np.abs(x)), float(abs(fe - rx) / np.dot(ref.residual_scale(), np.abs(x)))


# ------------------------------------------------------------------------------------------------------------------ GPU: every route
TWO_PASS_GENERIC = ("k_assemble_matrix<dump> + k_rows_from_tri", "k_assemble_matrix<dump> + k_rows_from_dense")
HEX27_MFMA = "k_hex27_dense_blocks + k_rows_from_tri"
TILED_KINDS = ("HEX8", "TET4", "QUAD4", "TRI3")
MARGINS = {}


def _record(key, err, bound):
    """the error as a fraction of the bar; printed at the end of the module (-s) for the record"""
    frac = float(err) / (BAR * float(bound)) if bound > 0 else (0.0 if err == 0 else np.inf)
    MARGINS[key] = max(MARGINS.get(key, 0.0), frac)
    return frac


def _assert_le(key, err, bound):
    frac = _record(key, err, bound)
    assert np.isfinite(err) and frac <= 1.0, (key, float(err), float(bound), frac)


@pytest.fixture(scope="module", autouse=True)
def _print_margins():
    yield
    if MARGINS:
        print("\nlargest error / bar per route and deformation:")
        for k in sorted(MARGINS):
            print(f"  {k:70s} {MARGINS[k]:.3f}")


def _builder(engine, m, model, w, p, u, lame):
    qt = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(lame)
    return (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(m).with_operator(fa.MaterialEllipticOperator(OPS[model]()))
            .with_quadrature_table(qt).with_u(u).build())


def _check_k(key, k, ref):
    kh = ref.csr_values(k.row_offsets, k.col_indices)
    vals = k.values.cpu().numpy() if hasattr(k.values, "cpu") else k.values
    _assert_le(key, np.abs(vals - kh).max(), np.abs(kh).max())
    return vals


def _assembled_routes(engine, asm, kind, model, ref, tag):
    """every assembled route of this kind; returns {route: values} for the rotation check"""
    import torch

    out = {}
    k = fa.CsrAssembler(fa.SCATTER_GATHER).assemble(asm)
    name = engine.last_kernel_name()
    if kind == "HEX27" and model == "NEO_HOOKEAN":
        assert name == HEX27_MFMA
        out["mfma"] = _check_k(f"K hex27 matrix cores {tag}", k, ref)
        engine.set_option("FENRIS_HIP_NO_MFMA", 1)
        k = fa.CsrAssembler(fa.SCATTER_GATHER).assemble(asm)
        assert engine.last_kernel_name() in TWO_PASS_GENERIC
        out["generic"] = _check_k(f"K hex27 no-mfma generic two-pass {tag}", k, ref)
        engine.set_option("FENRIS_HIP_NO_MFMA", None)
        return out
    assert name in TWO_PASS_GENERIC, name
    out["generic"] = _check_k(f"K {kind} generic two-pass {tag}", k, ref)
    if kind not in ("HEX8", "TET4"):
        return out
    engine.set_option("FENRIS_HIP_NO_TWO_PASS", 1)
    try:
        k = fa.CsrAssembler(fa.SCATTER_GATHER).assemble(asm)
        assert engine.last_kernel_name() == "k_assemble_matrix<gather>", engine.last_kernel_name()
        out["one-pass gather"] = _check_k(f"K {kind} one-pass gather {tag}", k, ref)
        k = fa.CsrAssembler(fa.SCATTER_ATOMIC).assemble(asm)
        assert engine.last_kernel_name() == "k_assemble_matrix<atomic>"
        out["atomic"] = _check_k(f"K {kind} one-pass atomic {tag}", k, ref)
        engine.color()
        k = fa.CsrAssembler(fa.SCATTER_COLORED).assemble(asm)
        assert engine.last_kernel_name() == "k_assemble_matrix<colored>"
        out["colored"] = _check_k(f"K {kind} one-pass colored {tag}", k, ref)
        # one row range: rows of nodes [lo, hi) only, the rest stays as it was
        nn = engine.num_nodes()
        lo, hi = nn // 3, (2 * nn) // 3
        ro = np.asarray(k.row_offsets).astype(np.int64)
        v = torch.zeros(len(k.col_indices), dtype=torch.float64, device="cuda")
        engine.assemble_matrix_rows(v, fa.SCATTER_GATHER, lo, hi)
        assert engine.last_kernel_name() == "k_assemble_matrix<gather>", engine.last_kernel_name()
        kh = ref.csr_values(k.row_offsets, k.col_indices)
        s = ref.s
        a, b = ro[s * lo], ro[s * hi]
        vr = v.cpu().numpy()
        _assert_le(f"K {kind} row range {tag}", np.abs(vr[a:b] - kh[a:b]).max(), np.abs(kh[a:b]).max())
        assert not np.any(vr[:a]) and not np.any(vr[b:])
    finally:
        engine.set_option("FENRIS_HIP_NO_TWO_PASS", None)
    return out


def _tangent_route(engine, asm, kind, ref, x, tag):
    t = fa.MatrixFreeTangent(asm)
    y = np.full(len(x), np.nan)
    t.apply(y, x)
    name = engine.last_kernel_name()
    assert name == ("k_tangent_tiled + k_operator_from_partials" if kind in TILED_KINDS else "k_mf_apply_elements + k_vector_from_elements_soa"), name
    yh, bound = ref.apply(x)
    _assert_le(f"apply {name.split()[0]} {kind} {tag}", np.abs(y - yh).max(), bound)
    d = t.diagonal()
    dh = ref.diagonal()
    _assert_le(f"diag {name.split()[0]} {kind} {tag}", np.abs(d - dh).max(), np.abs(dh).max())
    return y, d


def _shifted_route(engine, asm, kind, ref, x, tag):
    alpha, beta = 1.0, 2.0e-4   # backward Euler with dt^2 = 2e-4: both terms matter
    op = fa.MatrixFreeShiftedTangent(asm, RHO, alpha, beta)
    y = np.full(len(x), np.nan)
    op.apply(y, x)
    name = engine.last_kernel_name()
    if kind == "HEX8":
        assert name == "k_shifted_tangent_tiled + k_operator_from_partials", name
    else:
        assert "tiled" not in name, name
    yh, bound = ref.apply(x, alpha, beta)
    _assert_le(f"shifted apply {kind} {tag}", np.abs(y - yh).max(), bound)
    d = op.diagonal()
    dh = alpha * ref.diagonal("M") + beta * ref.diagonal()
    _assert_le(f"shifted diag {kind} {tag}", np.abs(d - dh).max(), np.abs(dh).max())


def _vector_routes(engine, asm, kind, ref, case, tag):
    """the residual and the energy on every route of the kind: the LDS-staged kernels, the tiles, and for Hex8 / Tet4 also the element pass
    without them"""
    if kind in TILED_KINDS:
        staged = "k_assemble_vector" if kind == "TRI3" else "k_assemble_vector_stream + k_vector_from_elements"
        routes = [("FENRIS_HIP_NO_ELEMENT_PASS", staged, "k_assemble_scalar"),
                  (None, "k_element_pass_tiled + k_vector_from_partials", "k_element_energy_tiled")]
        if kind in ("HEX8", "TET4"):
            routes.append(("FENRIS_HIP_NO_VECTOR_TILES", "k_element_pass + k_vector_from_elements_soa", "k_element_pass<scalar>"))
        # the one-pass scatter; the energy is a sum of partials whatever this switch says and stays on the tiles
        routes.append(("FENRIS_HIP_VECTOR_ATOMICS", "k_assemble_vector" if kind == "TRI3" else "k_assemble_vector_stream", "k_element_energy_tiled"))
    else:
        routes = [(None, "k_assemble_vector", "k_assemble_scalar")]
    for option, vname, ename in routes:
        if option:
            engine.set_option(option, 1)
        try:
            r = fa.VectorAssembler().assemble_vector(asm)
            assert engine.last_kernel_name() == vname, engine.last_kernel_name()
            _assert_le(f"residual {vname.split()[0]} {kind} {tag}", np.abs(r - ref.residual()).max(), ref.residual_scale(terms=(case == "e")).max())
            e = fa.assemble_scalar(asm)
            assert engine.last_kernel_name() == ename, engine.last_kernel_name()
            _assert_le(f"energy {ename} {kind} {tag}", abs(e - ref.energy()), ref.energy_scale(terms=(case == "e")))
        finally:
            if option:
                engine.set_option(option, None)
    return r, e


def _block_perm(R, n_nodes):
    """the signed permutation P = diag(R, R, ..) as (index, sign): (P v)[s I + i] = sign[i] v[s I + perm[i]]"""
    s = R.shape[0]
    perm = np.argmax(np.abs(R), axis=1)
    sign = R[np.arange(s), perm]
    idx = (s * np.arange(n_nodes)[:, None] + perm[None, :]).reshape(-1)
    return idx, np.tile(sign, n_nodes)


VARIANTS = ["HEX8_AFFINE", "HEX8_GENERAL", "TET4", "QUAD4", "TRI3", "TET10", "HEX27"]
GPU_CASES = [(v, c) for v in VARIANTS for c in ("a", "b", "e") + (("c", "d") if v in ("HEX8_AFFINE", "HEX8_GENERAL", "TET4") else ())]


@pytest.mark.gpu
@pytest.mark.parametrize("variant,case", GPU_CASES)
@pytest.mark.parametrize("model", ["NEO_HOOKEAN", "STVK"])
def test_large_deformation_against_long_double(variant, case, model):
    kind, m, w, p = mesh_of(variant)
    u = deformation(case, m.vertices)
    ref = reference(kind, model, m, w, p, u, case)
    tag = f"{variant} ({case}) {model}"
    eng = fa.Engine(0)
    try:
        asm = _builder(eng, m, model, w, p, u, lame_of(case))
        x = np.random.default_rng(7).standard_normal(len(u))
        ks = _assembled_routes(eng, asm, kind, model, ref, tag)
        y, d = _tangent_route(eng, asm, kind, ref, x, tag)
        if variant in ("HEX8_AFFINE", "HEX8_GENERAL", "TET10"):
            _shifted_route(eng, asm, kind, ref, x, tag)
        r, e = _vector_routes(eng, asm, kind, ref, case, tag)
        if case != "e":
            return
        # rotation invariance on the device alone: K(u_R) = P K(0) P^T, T(u_R) x = P T(0) P^T x, diag likewise; r(u_R) = 0 = psi(u_R)
        R = F3["e"] if m.vertices.shape[1] == 3 else F2["e"]
        idx, sign = _block_perm(R, m.num_nodes())
        ref0 = reference(kind, model, m, w, p, np.zeros_like(u), "e")
        eng.set_u(np.zeros_like(u))
        ks0 = _assembled_routes(eng, asm, kind, model, ref0, f"{variant} (0) {model}")
        for route, k_r in ks.items():
            k0 = k_rotated_from(ks0[route], ref0, idx, sign)
            _assert_le(f"rotation K {route} {kind} {model}", np.abs(k_r - k0).max(), np.abs(k0).max())
        xt = np.empty_like(x)
        xt[idx] = sign * x                                    # P^T x
        y0 = np.empty_like(x)
        fa.MatrixFreeTangent(asm).apply(y0, xt)
        _, bound = ref0.apply(xt)
        _assert_le(f"rotation apply {kind} {model}", np.abs(y - sign * y0[idx]).max(), bound)
        d0 = fa.MatrixFreeTangent(asm).diagonal()
        _assert_le(f"rotation diag {kind} {model}", np.abs(d - d0[idx]).max(), np.abs(d0).max())
        _assert_le(f"rotation residual {kind} {model}", np.abs(r).max(), ref.residual_scale(terms=True).max())
        _assert_le(f"rotation energy {kind} {model}", abs(e), ref.energy_scale(terms=True))
    finally:
        eng.close()


def k_rotated_from(k0_vals, ref0, idx, sign):
    """the CSR values of P K P^T on the same pattern: (P K P^T)[a][b] = sign[a] sign[b] K[idx[a]][idx[b]] (a signed permutation within each
    node block keeps the pattern)"""
    ro, ci = ref0.pattern()
    rows = np.repeat(np.arange(len(ro) - 1), np.diff(ro))
    key = idx[rows] * ref0.ndof + idx[ci]
    pos = np.searchsorted(ref0.pattern_keys, key)
    assert np.array_equal(ref0.pattern_keys[pos], key)
    return sign[rows] * sign[ci] * np.asarray(k0_vals)[pos]
