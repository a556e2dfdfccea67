"""The per-element expansion (fh_set_element_expansion, fh_set_thermal_expansion) on every route that carries it, against the long-double
reference of tests/expansion_reference.py, which applies the law to grad u at the quadrature points (the register-resident kernels apply it to
nodal values: the two forms are held to one reference).

Bars: those of tests/test_large_deformation.py for the same routes -- residual 1e-12 of its absolute scale (where r vanishes: of the magnitudes
of the terms of P), energy 1e-12 sum |psi_e|, apply 1e-12 || |K| |x| ||, diagonal 1e-12 max|d|; Newton solves against dense solves 1e-8 max|u|
with tolerance 1e-8 |f| and linear_rel_tol 1e-12 (tests/test_newton.py); difference quotients with step 1e-5 to 1e-7
(tests/test_tangent_operator.py)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import fenris_amd as fa
from fenris_amd import _ffi, quadrature
import dynamics_reference as dr
import expansion_reference as xr
import hp_reference as hp

BAR = 1e-12
LAME = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.3))
RHO = 2.5e3
OPS = {"LINEAR_ELASTIC": fa.LinearElasticMaterial, "NEO_HOOKEAN": fa.NeoHookeanMaterial, "STVK": fa.StVKMaterial,
       "STABLE_NEO_HOOKEAN": fa.StableNeoHookeanMaterial}
MODELS = list(OPS)
LINEAR_KINDS = ["HEX8", "TET4", "QUAD4", "TRI3"]
QUADRATIC_KINDS = ["TET10", "HEX20", "HEX27", "TRI6", "QUAD9"]
KINDS = LINEAR_KINDS + QUADRATIC_KINDS
FH_UNSUPPORTED, FH_BAD_ARGUMENT, FH_INVALID_STATE = _ffi.FH_UNSUPPORTED, _ffi.FH_BAD_ARGUMENT, _ffi.FH_INVALID_STATE


# ------------------------------------------------------------------------------------------------------------------ meshes and assemblers
def _jitter(m, amp, seed, keep=None):
    v = m.vertices + amp * np.random.default_rng(seed).uniform(-1.0, 1.0, m.vertices.shape)
    if keep is not None:
        v[keep] = m.vertices[keep]
    return fa.Mesh(v, m.connectivity, m.elem_kind)


def small_mesh(kind, seed=5):
    """(mesh, weights, points): 2^d elements of the cube kinds, the smallest box mesh of the simplices (8 triangles, 12 tetrahedra), jittered
    so that no hexahedron or quadrilateral is affine; the quadratic kinds are built on the jittered linear mesh"""
    if kind in ("HEX8", "HEX20", "HEX27"):
        m = _jitter(fa.procedural.create_rectangular_uniform_hex_mesh(0.5, 2, 2, 2, 1), 0.03, seed)
        if kind == "HEX8":
            return m, *map(np.asarray, quadrature.tensor.hexahedron_gauss(2))
        return (fa.hex20_mesh_from_hex8(m) if kind == "HEX20" else fa.hex27_mesh_from_hex8(m)), *map(np.asarray, quadrature.tensor.hexahedron_gauss(3))
    if kind in ("TET4", "TET10"):
        m = _jitter(fa.procedural.create_unit_box_uniform_tet_mesh_3d(1), 0.03, seed)
        return (m if kind == "TET4" else fa.tet10_mesh_from_tet4(m)), *map(np.asarray, quadrature.total_order.tetrahedron(2))
    if kind in ("QUAD4", "QUAD9"):
        m = _jitter(fa.procedural.create_unit_square_uniform_quad_mesh_2d(2), 0.03, seed)
        if kind == "QUAD4":
            return m, *map(np.asarray, quadrature.tensor.quadrilateral_gauss(2))
        return fa.quad9_mesh_from_quad4(m), *map(np.asarray, quadrature.tensor.quadrilateral_gauss(3))
    m = _jitter(fa.procedural.create_unit_square_uniform_tri_mesh_2d(2), 0.03, seed)
    return (m if kind == "TRI3" else fa.tri6_mesh_from_tri3(m)), *map(np.asarray, quadrature.total_order.triangle(2))


def assembler(engine, m, model, w, p, u):
    qt = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(LAME)
    return (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(m).with_operator(fa.MaterialEllipticOperator(OPS[model]()))
            .with_quadrature_table(qt).with_u(u).build())


def reference(kind, model, m, w, p, u, theta, conn=None):
    return xr.Reference(kind, model, m.vertices, m.connectivity if conn is None else conn, w, p, u, LAME.mu, LAME.lambda_, theta, rho=RHO)


def random_u(m, amp=0.05, seed=1):
    """a smooth field plus noise with gradients of about `amp` (the element size is ~0.5)"""
    X = m.vertices
    rng = np.random.default_rng(seed)
    A = rng.uniform(-amp, amp, (X.shape[1], X.shape[1]))
    return (X @ A.T + 0.2 * amp * 0.5 * rng.uniform(-1.0, 1.0, X.shape)).reshape(-1)


def random_theta(m, seed=2, lo=0.9, hi=1.1):
    return np.random.default_rng(seed).uniform(lo, hi, m.num_elements())


@pytest.fixture()
def engine():
    eng = fa.Engine(0)
    yield eng
    eng.close()


def _le(err, bound, what):
    assert np.isfinite(err) and err <= BAR * bound, (what, float(err), float(bound), float(err / bound) if bound else np.inf)


def check_vector_routes(engine, asm, ref, vanishing, what):
    r = fa.VectorAssembler().assemble_vector(asm)
    _le(np.abs(r - ref.residual()).max(), ref.residual_scale(terms=vanishing).max(), ("residual", what, engine.last_kernel_name()))
    e = fa.assemble_scalar(asm)
    _le(abs(e - ref.energy()), ref.energy_scale(terms=vanishing), ("energy", what, engine.last_kernel_name()))
    return r, e


def check_tangent_routes(engine, asm, ref, x, what, shifted=True):
    t = fa.MatrixFreeTangent(asm)
    y = np.full(len(x), np.nan)
    t.apply(y, x)
    yh, bound = ref.apply(x)
    _le(np.abs(y - yh).max(), bound, ("apply", what, engine.last_kernel_name()))
    d = t.diagonal()
    _le(np.abs(d - ref.diagonal()).max(), np.abs(ref.diagonal()).max(), ("diagonal", what, engine.last_kernel_name()))
    out = [y, d]
    if shifted:
        alpha, beta = 1.0, 0.01
        op = fa.MatrixFreeShiftedTangent(asm, RHO, alpha, beta)
        ys = np.full(len(x), np.nan)
        op.apply(ys, x)
        yh, bound = ref.apply(x, alpha, beta)
        _le(np.abs(ys - yh).max(), bound, ("shifted apply", what, engine.last_kernel_name()))
        ds = op.diagonal()
        dh = alpha * ref.diagonal("M") + beta * ref.diagonal()
        _le(np.abs(ds - dh).max(), np.abs(dh).max(), ("shifted diagonal", what, engine.last_kernel_name()))
        out += [ys, ds]
    return out


# ------------------------------------------------------------------------------------------------------------------ 11. the reference itself
@pytest.mark.parametrize("kind", ["TRI6", "QUAD9", "HEX20"])
def test_added_shape_functions_pin_the_oracle_node_order(oracle, kind):
    n, d = xr.EXTRA_KINDS[kind]
    for xi in np.random.default_rng(1).uniform(-1.0, 0.4, (7, d)):
        phi, g = xr.shape(kind, xi)
        assert phi.dtype == np.longdouble and g.shape == (n, d)
        assert np.abs(oracle.element_gradients(getattr(oracle, kind), xi).T - g.astype(np.float64)).max() <= 1e-15
        assert np.abs(oracle.element_basis(getattr(oracle, kind), xi) - phi.astype(np.float64)).max() <= 1e-15


@pytest.mark.parametrize("kind", ["HEX8", "TRI3", "TET10", "QUAD9"])
@pytest.mark.parametrize("model", MODELS)
def test_reference_residual_is_the_gradient_of_its_energy(kind, model):
    """r . x = (E(u + h x) - E(u - h x)) / 2h and K x = (r(u + h x) - r(u - h x)) / 2h in long double under a random field"""
    m, w, p = small_mesh(kind)
    theta = random_theta(m)
    ld = np.longdouble
    u = random_u(m).astype(ld)
    x = np.random.default_rng(3).standard_normal(u.size).astype(ld)
    h = ld(1e-7)
    ref, rp, rm = (reference(kind, model, m, w, p, v, theta) for v in (u, u + h * x, u - h * x))
    rx = np.dot(ref.residual(), x)
    fe = (rp.energy() - rm.energy()) / (2 * h)
    assert abs(fe - rx) <= 1e-9 * np.dot(ref.residual_scale(), np.abs(x)), float(abs(fe - rx) / np.dot(ref.residual_scale(), np.abs(x)))
    kx = ref.apply(x)[0]
    fd = (rp.residual() - rm.residual()) / (2 * h)
    assert np.abs(fd - kx).max() <= 1e-9 * np.abs(kx).max(), float(np.abs(fd - kx).max() / np.abs(kx).max())


@pytest.mark.parametrize("kind", ["HEX8", "QUAD4"])
@pytest.mark.parametrize("model", ["NEO_HOOKEAN", "STVK", "STABLE_NEO_HOOKEAN"])
def test_multiplicative_law_linearises_to_the_additive_one(kind, model):
    """with theta = 1 + t and u = t v the hyperelastic residual is the linear-elastic one to first order: the difference falls like t^2.
    (Stable Neo-Hookean linearises to the Lame pair its own parameters come from.)"""
    m, w, p = small_mesh(kind)
    d = m.vertices.shape[1]
    mu, lam = (xr.snh.parameters(d, LAME.mu, LAME.lambda_) if model == "STABLE_NEO_HOOKEAN" else (LAME.mu, LAME.lambda_))
    g = np.random.default_rng(4).uniform(-1.0, 1.0, m.num_elements())
    v = random_u(m, amp=1.0)
    gaps = []
    for t in (1e-3, 1e-4):
        args = (m.vertices, m.connectivity, w, p, t * v)
        rh = xr.Reference(kind, model, *args, mu, lam, 1.0 + t * g).residual()
        rl = xr.Reference(kind, "LINEAR_ELASTIC", *args, LAME.mu, LAME.lambda_, 1.0 + t * g).residual()
        gaps.append(float(np.abs(rh - rl).max() / np.abs(rl).max()))
    # the residuals are of first order in t and their difference of second: a t ten times smaller, a relative gap about ten times smaller
    assert gaps[0] <= 0.05 and gaps[1] <= 0.2 * gaps[0], gaps


def test_thermal_stretch_formula():
    conn = np.array([[0, 1, 2], [1, 2, 3]])
    th = xr.thermal_stretches(conn, [10.0, 20.0, 30.0, 70.0], [1e-3, 2e-3], 20.0)
    assert np.allclose(th, [1.0, 1.0 + 2e-3 * 20.0], rtol=1e-15)


# ------------------------------------------------------------------------------------------------------------------ 1. free expansion
@pytest.mark.gpu
@pytest.mark.parametrize("theta", [0.9, 1.2])
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("kind", KINDS)
def test_free_expansion_is_stress_free(engine, kind, model, theta):
    m, w, p = small_mesh(kind)
    u = ((theta - 1.0) * m.vertices).reshape(-1)
    asm = assembler(engine, m, model, w, p, u)
    engine.set_element_expansion(theta)
    ref = reference(kind, model, m, w, p, u, theta)
    r, e = check_vector_routes(engine, asm, ref, True, (kind, model, theta))
    # ... and absolutely: the residual and the energy are rounding noise of their terms
    assert np.abs(r).max() <= BAR * ref.residual_scale(terms=True).max() and abs(e) <= BAR * ref.energy_scale(terms=True)


# ------------------------------------------------------------------------------------------------------------------ 2. parity
@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("kind", KINDS)
def test_parity_with_the_reference(engine, kind, model):
    m, w, p = small_mesh(kind)
    u, theta = random_u(m), random_theta(m)
    asm = assembler(engine, m, model, w, p, u)
    engine.set_element_expansion(theta)
    assert np.array_equal(engine.element_expansion(), theta)
    ref = reference(kind, model, m, w, p, u, theta)
    assert ref.det_F_min > 0.0
    check_vector_routes(engine, asm, ref, False, (kind, model))
    x = np.random.default_rng(7).standard_normal(len(u))
    check_tangent_routes(engine, asm, ref, x, (kind, model))
    # the field matters: without it the residual is another one
    engine.set_element_expansion(None)
    r0 = fa.VectorAssembler().assemble_vector(asm)
    assert np.abs(r0 - ref.residual()).max() > 1e-3 * ref.residual_scale().max()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["HEX8", "TET4"])
@pytest.mark.parametrize("option", ["FENRIS_HIP_NO_VECTOR_TILES", "FENRIS_HIP_NO_ELEMENT_PASS", "FENRIS_HIP_VECTOR_ATOMICS"])
def test_parity_off_the_tiles(engine, kind, option):
    """the element pass without tiles, the LDS-staged kernels and the per-element matrix-free kernels of the linear kinds"""
    m, w, p = small_mesh(kind)
    u, theta = random_u(m), random_theta(m)
    x = np.random.default_rng(7).standard_normal(len(u))
    for model in ("LINEAR_ELASTIC", "NEO_HOOKEAN"):
        asm = assembler(engine, m, model, w, p, u)
        engine.set_element_expansion(theta)
        ref = reference(kind, model, m, w, p, u, theta)
        engine.set_option(option, 1)
        try:
            check_vector_routes(engine, asm, ref, False, (kind, model, option))
            assert "tiled" not in engine.last_kernel_name() or option == "FENRIS_HIP_VECTOR_ATOMICS"
            check_tangent_routes(engine, asm, ref, x, (kind, model, option))
        finally:
            engine.set_option(option, None)


@pytest.mark.gpu
def test_compact_table_and_uniform_count(engine):
    """per-element parameters (rule_map) beside the field; count == 1 is the field of E equal stretches"""
    m, w, p = small_mesh("HEX8")
    u = random_u(m)
    asm = assembler(engine, m, "STVK", w, p, u)
    engine.set_element_expansion(1.07)
    assert np.array_equal(engine.element_expansion(), np.full(m.num_elements(), 1.07))
    r1 = fa.VectorAssembler().assemble_vector(asm)
    engine.set_element_expansion(np.full(m.num_elements(), 1.07))
    assert np.array_equal(fa.VectorAssembler().assemble_vector(asm), r1)
    # a compact table (rule_map) whose two rules hold the same parameters: the reference of the uniform table, on the tiles and off them
    E = m.num_elements()
    qt = fa.CompactQuadratureTable(p, w, [LAME, LAME], np.arange(E) % 2)
    theta = random_theta(m)
    ref = reference("HEX8", "STVK", m, w, p, u, theta)
    x = np.random.default_rng(7).standard_normal(len(u))
    for option in (None, "FENRIS_HIP_NO_VECTOR_TILES", "FENRIS_HIP_NO_ELEMENT_PASS"):
        asm2 = (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(m).with_operator(fa.MaterialEllipticOperator(fa.StVKMaterial()))
                .with_quadrature_table(qt).with_u(u).build())
        engine.set_element_expansion(theta)
        if option:
            engine.set_option(option, 1)
        try:
            check_vector_routes(engine, asm2, ref, False, ("compact table", option))
            check_tangent_routes(engine, asm2, ref, x, ("compact table", option), shifted=False)
        finally:
            if option:
                engine.set_option(option, None)


# ------------------------------------------------------------------------------------------------------------------ 3. tile corners
def _corner_mesh(which):
    if which == "HEX8":
        return _jitter(fa.procedural.create_rectangular_uniform_hex_mesh(1.0, 5, 6, 10, 1), 0.05, 11), *map(np.asarray, quadrature.tensor.hexahedron_gauss(2))
    if which == "HEX8_AXIS_ALIGNED":
        return fa.procedural.create_rectangular_uniform_hex_mesh(1.0, 5, 6, 10, 1), *map(np.asarray, quadrature.tensor.hexahedron_gauss(2))
    return _jitter(fa.procedural.create_unit_box_uniform_tet_mesh_3d(3), 0.01, 12), *map(np.asarray, quadrature.total_order.tetrahedron(2))   # 324


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("which,model", [("HEX8", "NEO_HOOKEAN"), ("HEX8", "LINEAR_ELASTIC"), ("TET4", "STVK"), ("TET4", "LINEAR_ELASTIC"),
                                         ("HEX8_AXIS_ALIGNED", "LINEAR_ELASTIC"), ("HEX8_AXIS_ALIGNED", "STABLE_NEO_HOOKEAN")])
def test_tile_corners(engine, which, model, masked):
    """more than one tile of 256 elements, the last one ragged; under a mask that leaves elements of both tiles live and dead.  The
    axis-aligned Hex8 mesh with linear elasticity and a symmetric rule takes the quadrature-free moment form with a field set."""
    kind = which.split("_")[0]
    m, w, p = _corner_mesh(which)
    E = m.num_elements()
    assert E > 256
    u, theta = random_u(m, amp=0.05), random_theta(m, seed=21)
    asm = assembler(engine, m, model, w, p, u)
    engine.set_element_expansion(theta)
    conn, th = m.connectivity, theta
    if masked:
        mask = np.random.default_rng(22).uniform(size=E) < 0.7
        engine.set_active_elements(mask.astype(np.uint8))
        conn, th = m.connectivity[mask], theta[mask]
    ref = reference(kind, model, m, w, p, u, th, conn=conn)
    check_vector_routes(engine, asm, ref, False, (which, model, masked))
    assert engine.last_kernel_name() == "k_element_energy_tiled"
    x = np.random.default_rng(7).standard_normal(len(u))
    check_tangent_routes(engine, asm, ref, x, (which, model, masked), shifted=False)
    if which == "HEX8_AXIS_ALIGNED" and model == "LINEAR_ELASTIC":
        # the residual above came from the moment form: with that form switched off the point loop of the monomial form runs, which sums in
        # another order -- within the bar as well, and not the same bits (a silent fall-back to the point loop would give equal bits)
        r_moment = fa.VectorAssembler().assemble_vector(asm)
        engine.set_option("FENRIS_HIP_NO_MOMENT_RESIDUAL", 1)
        try:
            r_points = fa.VectorAssembler().assemble_vector(asm)
        finally:
            engine.set_option("FENRIS_HIP_NO_MOMENT_RESIDUAL", None)
        assert engine.last_kernel_name() == "k_element_pass_tiled + k_vector_from_partials"
        _le(np.abs(r_points - ref.residual()).max(), ref.residual_scale().max(), ("residual, point loop", which, masked))
        assert not np.array_equal(r_moment, r_points)


# ------------------------------------------------------------------------------------------------------------------ 4. bits
def _ordered_residual_norm(asm):
    """|r(u)| at the assembler's u through the residual's ordered route (the one Newton and the integrators take): the norm a Newton solve
    reports before its first step"""
    clamp = np.where(asm.space.vertices[:, 0] < 0.1)[0]
    try:
        res = fa.MatrixFreeNewton(asm).with_dirichlet_nodes(clamp).solve(np.array(asm.u_host, dtype=np.float64), fa.NewtonSettings(1, 1e-300))
    except fa.NewtonError as e:
        res = e.result
    asm.with_u(asm.u_host)
    return np.array([res.initial_residual_norm])


def _all_routes(engine, asm, x, kind):
    """fh_assemble_vector of the quadratic kinds scatters with floating-point atomics, a route that does not promise to repeat its own bits:
    those kinds enter the comparison through the ordered route of the residual instead"""
    out = [fa.VectorAssembler().assemble_vector(asm) if kind in LINEAR_KINDS else _ordered_residual_norm(asm), np.array([fa.assemble_scalar(asm)])]
    t = fa.MatrixFreeTangent(asm)
    y = np.zeros(len(x))
    t.apply(y, x)
    out += [y, t.diagonal()]
    op = fa.MatrixFreeShiftedTangent(asm, RHO, 1.0, 0.01)
    ys = np.zeros(len(x))
    op.apply(ys, x)
    out += [ys, op.diagonal()]
    return out


def _same_bits(before, after):
    for i, (a, b) in enumerate(zip(before, after)):
        assert np.array_equal(a, b), i


def _newton3(asm, m, f):
    clamp = np.where(m.vertices[:, 0] < 0.1)[0]
    u = np.zeros(len(f))
    try:
        fa.MatrixFreeNewton(asm).with_dirichlet_nodes(clamp).with_load(f).solve(u, fa.NewtonSettings(3, 1e-30), linear_rel_tol=1e-10)
    except fa.MaximumIterationsReached:
        pass
    return u


@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("kind", ["HEX8", "TET4", "QUAD4", "TRI3", "TET10", "HEX27"])
def test_a_field_of_ones_and_a_cleared_field_give_the_bits_of_no_field(engine, kind, model):
    m, w, p = small_mesh(kind)
    u = random_u(m)
    x = np.random.default_rng(7).standard_normal(len(u))
    f = 1e2 * np.random.default_rng(8).standard_normal(len(u))
    asm = assembler(engine, m, model, w, p, u)
    asm.u_host = u
    never = _all_routes(engine, asm, x, kind)
    asm.with_u(np.zeros(len(u)))
    never_n = _newton3(asm, m, f)
    for field in (np.ones(m.num_elements()), 1.0):
        asm.with_u(u)
        engine.set_element_expansion(field)
        _same_bits(never, _all_routes(engine, asm, x, kind))
        asm.with_u(np.zeros(len(u)))
        assert np.array_equal(_newton3(asm, m, f), never_n)
    # set, then cleared
    asm.with_u(u)
    engine.set_element_expansion(random_theta(m))
    first = _all_routes(engine, asm, x, kind)
    second = _all_routes(engine, asm, x, kind)
    assert not np.array_equal(first[0], never[0])
    _same_bits(first, second)   # two runs with the same field
    engine.set_element_expansion(None)
    _same_bits(never, _all_routes(engine, asm, x, kind))
    asm.with_u(np.zeros(len(u)))
    assert np.array_equal(_newton3(asm, m, f), never_n)


# ------------------------------------------------------------------------------------------------------------------ 5. consistency
@pytest.mark.gpu
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("kind", ["HEX8", "TET4", "QUAD9"])
def test_energy_residual_and_tangent_are_consistent_on_the_device(engine, kind, model):
    """central differences of the device energy give the device residual, of the device residual the tangent apply: step 1e-5 and bar 1e-7,
    those of tests/test_tangent_operator.py::test_tangent_is_the_derivative_of_the_residual.  The energy's quotient also carries the rounding of
    the two energies it subtracts, 2 eps sum |psi_e| / (2 step)."""
    m, w, p = small_mesh(kind)
    u, theta = random_u(m, amp=0.1), random_theta(m)
    asm = assembler(engine, m, model, w, p, u)
    engine.set_element_expansion(theta)
    x = 0.1 * np.random.default_rng(1).standard_normal(len(u))
    eps = 1e-5

    def residual(v):
        asm.with_u(v)
        return fa.VectorAssembler().assemble_vector(asm)

    def energy(v):
        asm.with_u(v)
        return fa.assemble_scalar(asm)

    r = residual(u)
    y = np.zeros(len(u))
    fa.MatrixFreeTangent(asm).apply(y, x)
    fd = (residual(u + eps * x) - residual(u - eps * x)) / (2 * eps)
    assert np.abs(y - fd).max() <= 1e-7 * np.abs(y).max(), np.abs(y - fd).max() / np.abs(y).max()
    fe = (energy(u + eps * x) - energy(u - eps * x)) / (2 * eps)
    scale = reference(kind, model, m, w, p, u, theta).energy_scale(terms=True)
    bound = 1e-7 * np.dot(np.abs(r), np.abs(x)) + 2.0 * np.finfo(float).eps * float(scale) / (2 * eps)
    assert abs(fe - np.dot(r, x)) <= bound, (abs(fe - np.dot(r, x)), bound)


# ------------------------------------------------------------------------------------------------------------------ 6. thermal stress
def _block(n=3):
    """a Hex8 block of n^3 elements on [0, 1]^3 with jittered interior nodes (the faces stay planes)"""
    m = fa.procedural.create_rectangular_uniform_hex_mesh(1.0, 1, 1, 1, n)
    X = m.vertices
    boundary = np.where(((X < 1e-9) | (X > 1.0 - 1e-9)).any(axis=1))[0]
    return _jitter(m, 0.05, 31, keep=boundary)


def _faces(X, released_top):
    """(nodes, axis) of the roller faces: both faces of every axis; released_top: not the face z = 1 (the face z = 0 keeps holding the rigid
    translation along z, which a released pair of faces would leave free)"""
    return [(np.where((X[:, ax] < 1e-9) | ((X[:, ax] > 1.0 - 1e-9) & (not (released_top and ax == 2))))[0], ax) for ax in range(3)]


def _rollers(solver, X, released_top):
    for face, ax in _faces(X, released_top):
        solver = solver.with_dirichlet_dofs(face, [ax])
    return solver


def _fixed_dofs(X, released_top):
    return np.unique(np.concatenate([3 * face + ax for face, ax in _faces(X, released_top)]))


@pytest.mark.gpu
@pytest.mark.parametrize("theta", [1.01, 0.98])
def test_confined_block_carries_the_analytic_thermal_stress(engine, theta):
    m = _block()
    w, p = map(np.asarray, quadrature.tensor.hexahedron_gauss(2))
    n = 3 * m.num_nodes()
    asm = assembler(engine, m, "LINEAR_ELASTIC", w, p, np.zeros(n))
    engine.set_element_expansion(theta)
    want = -(3.0 * LAME.lambda_ + 2.0 * LAME.mu) * (theta - 1.0)
    for quantity in ("cauchy_stress", "stress_pk1"):
        for where in ("points", "elements", "nodes"):
            s = engine.recover(quantity, where).cpu().numpy()
            assert np.abs(s - want * np.eye(3)[None]).max() <= BAR * abs(want) * 10, (quantity, where)   # (ten terms of that size per entry)
    assert np.abs(engine.recover("von_mises", "points").cpu().numpy()).max() <= BAR * abs(want) * 10
    psi = engine.recover("energy_density", "elements").cpu().numpy()
    assert np.abs(psi - 1.5 * abs(want) * abs(theta - 1.0)).max() <= BAR * 10 * abs(want) * abs(theta - 1.0)
    assert np.abs(engine.recover("strain", "points").cpu().numpy()).max() == 0.0 and np.abs(engine.recover("grad_u", "points").cpu().numpy()).max() == 0.0
    # every face on rollers: u = 0 solves the problem
    ref = reference("HEX8", "LINEAR_ELASTIC", m, w, p, np.zeros(n), theta)
    f_th = ref.thermal_load().astype(np.float64)
    tol = 1e-8 * np.linalg.norm(f_th)
    u = np.zeros(n)
    res = _rollers(fa.MatrixFreeNewton(asm), m.vertices, False).solve(u, fa.NewtonSettings(20, tol), linear_rel_tol=1e-12)
    assert res.residual_norm <= tol and res.iterations == 0 and not np.any(u)
    # the face z = 1 released: the dense solve K u = f_th
    fixed = _fixed_dofs(m.vertices, True)
    uh = ref.solve_linear(fixed)
    u = np.zeros(n)
    asm.with_u(u)
    res = _rollers(fa.MatrixFreeNewton(asm), m.vertices, True).solve(u, fa.NewtonSettings(20, tol), linear_rel_tol=1e-12)
    assert res.residual_norm <= tol
    assert np.abs(u - uh).max() <= 1e-8 * np.abs(uh).max(), np.abs(u - uh).max() / np.abs(uh).max()
    assert np.abs(uh).max() > 1e-3 * abs(theta - 1.0)


# ------------------------------------------------------------------------------------------------------------------ 7. bimetal strip
@pytest.mark.gpu
def test_bimetal_strip_bends_as_the_dense_solve_says(engine):
    m = _jitter(fa.procedural.create_rectangular_uniform_hex_mesh(1.0, 16, 2, 2, 1), 0.05, 41)
    w, p = map(np.asarray, quadrature.tensor.hexahedron_gauss(2))
    X, n = m.vertices, 3 * m.num_nodes()
    zc = X[m.connectivity.astype(np.int64)][:, :, 2].mean(axis=1)
    alpha = np.where(zc < 1.0, 1.2e-5, 2.3e-5)
    T, T_ref = 20.0 + 15.0 * X[:, 0], 20.0
    asm = assembler(engine, m, "LINEAR_ELASTIC", w, p, np.zeros(n))
    engine.set_thermal_expansion(T, alpha, T_ref)
    assert engine.last_kernel_name() == "k_thermal_stretch"
    theta = engine.element_expansion()
    want = xr.thermal_stretches(m.connectivity, T, alpha, T_ref)
    # the same sums in the same order; the device may contract 1 + alpha (mean - T_ref) into one fma: an ulp of theta
    assert np.abs(theta - want).max() <= 2.0 * np.finfo(float).eps * np.abs(want).max()
    ref = reference("HEX8", "LINEAR_ELASTIC", m, w, p, np.zeros(n), theta)
    f_th = ref.thermal_load()
    _le(np.abs(engine.thermal_load() - f_th).max(), ref.residual_scale(terms=True).max(), "thermal load")
    clamp = np.where(X[:, 0] < X[:, 0].min() + 0.2)[0]
    fixed = (3 * clamp[:, None] + np.arange(3)[None, :]).reshape(-1)
    uh = ref.solve_linear(fixed)
    tol = 1e-8 * np.linalg.norm(f_th.astype(np.float64))
    u = np.zeros(n)
    res = fa.MatrixFreeNewton(asm).with_dirichlet_nodes(clamp).solve(u, fa.NewtonSettings(20, tol), linear_rel_tol=1e-12, linear_max_iter=20000)
    assert res.residual_norm <= tol
    assert np.abs(u - uh).max() <= 1e-8 * np.abs(uh).max(), np.abs(u - uh).max() / np.abs(uh).max()
    tip = np.where(X[:, 0] > X[:, 0].max() - 0.2)[0]
    assert abs(u[3 * tip + 2].mean()) > 10.0 * abs(u[3 * tip + 1].mean())   # it bends across the layers
    # a scalar alpha and the uniform temperature: no expansion
    engine.set_thermal_expansion(np.full(m.num_nodes(), T_ref), 1e-5, T_ref)
    assert np.array_equal(engine.element_expansion(), np.ones(m.num_elements()))


# ------------------------------------------------------------------------------------------------------------------ 8. integrators
class _Problem(dr.Problem):
    """dynamics_reference.Problem with the residual, energy, tangent and mass of the expansion reference (long double, rounded to doubles)"""

    def __init__(self, kind, model, m, w, p, theta, dirichlet, rho):
        self.kind, self.model, self.m, self.w, self.p, self.theta = kind, model, m, w, p, theta
        self.d = self.s = m.vertices.shape[1]
        self.N = m.num_nodes()
        self.n = self.s * self.N
        self.free = np.ones(self.n, dtype=bool)
        for k in range(self.s):
            self.free[self.s * np.asarray(dirichlet, dtype=np.int64) + k] = False
        self.f, self.load_factor, self.direct, self.rho = np.zeros(self.n), None, "dense", rho
        self._mass = None

    def _ref(self, u):
        return xr.Reference(self.kind, self.model, self.m.vertices, self.m.connectivity, self.w, self.p, u, LAME.mu, LAME.lambda_, self.theta, rho=self.rho)

    def residual(self, u):
        return self._ref(u).residual().astype(np.float64)

    def energy(self, u):
        return float(self._ref(u).energy())

    def _dense(self, ref, elem):
        rows, cols = np.divmod(ref.pattern_keys, ref.ndof)
        return sp.csr_matrix((ref._on_pattern(elem).astype(np.float64), (rows, cols)), shape=(self.n, self.n))

    def tangent(self, u):
        ref = self._ref(u)
        return self._dense(ref, ref.ke)

    def mass(self):
        if self._mass is None:
            ref = self._ref(np.zeros(self.n))
            self._mass = self._dense(ref, ref.me)
        return self._mass


def _dynamics_case(engine, model="NEO_HOOKEAN"):
    m, w, p = small_mesh("HEX8")
    clamp = np.where(m.vertices[:, 0] < 0.1)[0]
    theta = random_theta(m, lo=0.97, hi=1.03)
    n = 3 * m.num_nodes()
    asm = assembler(engine, m, model, w, p, np.zeros(n))
    return m, w, p, clamp, theta, n, asm


@pytest.mark.gpu
def test_central_differences_from_rest_follow_the_reference(engine):
    """five steps from rest: the field alone sets the body in motion.  Rounding only on both sides (the reference's residual is long double):
    1e-10, the bar of tests/test_dynamics.py's central-difference runs of that length"""
    m, w, p, clamp, theta, n, asm = _dynamics_case(engine)
    dt = 2e-5
    prob = _Problem("HEX8", "NEO_HOOKEAN", m, w, p, theta, clamp, RHO)
    uh, vh, ah, rech = dr.central_difference(prob, np.zeros(n), np.zeros(n), dt, 5, 0)
    ti = fa.CentralDifference(asm, RHO, dt).with_dirichlet_nodes(clamp).with_element_expansion(theta)
    ti.set_state(np.zeros(n))
    rec = ti.step(5)
    u, v, a, time, step = ti.state()
    assert step == 5 and np.abs(uh).max() > 0.0
    for got, want in ((u, uh), (v, vh), (a, ah)):
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max(), np.abs(got - want).max() / np.abs(want).max()
    assert abs(rec.kinetic[-1] - rech[-1][0]) <= 1e-10 * abs(rech[-1][0]) and abs(rec.stored[-1] - rech[-1][1]) <= 1e-10 * abs(rech[-1][1])
    # cut into two calls: the uncut run bit for bit
    ti.set_state(np.zeros(n))
    ti.step(2)
    ti.step(3)
    for got, want in zip(ti.state()[:3], (u, v, a)):
        assert np.array_equal(got, want)
    # the stable step sees the field: dt_crit of the hyperelastic tangent at the strained state differs from the one without it
    om, dtc = ti.stable_dt()
    ti.with_element_expansion(None)
    om0, _ = ti.stable_dt()
    assert om > 0.0 and dtc == 2.0 / om and om != om0


@pytest.mark.gpu
def test_backward_euler_from_rest_follows_the_reference(engine):
    """three steps from rest, Newton to 1e-11 |M a_0| dt^2-sized residuals on both sides and linear_rel_tol 1e-12: 1e-8, the bar of the Newton
    tests against dense solves"""
    m, w, p, clamp, theta, n, asm = _dynamics_case(engine)
    dt = 1e-3
    prob = _Problem("HEX8", "NEO_HOOKEAN", m, w, p, theta, clamp, RHO)
    tol = 1e-10 * np.linalg.norm(prob.residual(np.zeros(n))[prob.free]) * dt * dt
    st, uh, vh, ah, rech, done, _ = dr.implicit(prob, "euler", np.zeros(n), np.zeros(n), dt, 3, 0, tol=tol)
    assert st == "ok" and done == 3
    ti = (fa.BackwardEuler(asm, RHO, dt).with_newton(fa.NewtonSettings(None, tol), linear_rel_tol=1e-12).with_dirichlet_nodes(clamp)
          .with_element_expansion(theta))
    ti.set_state(np.zeros(n))
    ti.step(3)
    u, v, a, time, step = ti.state()
    assert step == 3 and np.abs(uh).max() > 0.0
    for got, want in ((u, uh), (v, vh)):
        assert np.abs(got - want).max() <= 1e-8 * np.abs(want).max(), np.abs(got - want).max() / np.abs(want).max()
    ti.set_state(np.zeros(n))
    ti.step(1)
    ti.step(2)
    for got, want in zip(ti.state()[:3], (u, v, a)):
        assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------------ 9. context reuse
@pytest.mark.gpu
@pytest.mark.parametrize("model", ["LINEAR_ELASTIC", "NEO_HOOKEAN"])
def test_a_reused_context_answers_like_a_fresh_one(model):
    m, w, p = small_mesh("HEX8")
    clamp = np.where(m.vertices[:, 0] < 0.1)[0]
    n = 3 * m.num_nodes()
    theta = random_theta(m, lo=0.97, hi=1.03)
    f = 1e2 * np.random.default_rng(8).standard_normal(n)
    x = np.random.default_rng(7).standard_normal(n)
    u_mid = random_u(m)

    def answers(eng, asm, field):
        """a Newton solve from zero, then the tangent with its Dirichlet scale at u_mid, then the stable step"""
        eng.set_element_expansion(field)
        asm.with_u(np.zeros(n))
        u = np.zeros(n)
        fa.MatrixFreeNewton(asm).with_dirichlet_nodes(clamp).with_load(f).solve(u, fa.NewtonSettings(30, 1e-8 * np.linalg.norm(f)), linear_rel_tol=1e-12)
        asm.with_u(u_mid)
        t = fa.MatrixFreeTangent(asm).with_dirichlet_nodes(clamp)
        y = np.zeros(n)
        t.apply(y, x)
        ti = fa.CentralDifference(asm, RHO, 1e-5).with_dirichlet_nodes(clamp)
        ti.set_state(u_mid)
        return [u, y, t.diagonal(), np.array(ti.stable_dt())]

    def fresh(field):
        eng = fa.Engine(0)
        try:
            return answers(eng, assembler(eng, m, model, w, p, np.zeros(n)), field)
        finally:
            eng.close()

    eng = fa.Engine(0)
    try:
        asm = assembler(eng, m, model, w, p, np.zeros(n))
        with_field = answers(eng, asm, theta)
        without = answers(eng, asm, None)
        again = answers(eng, asm, theta)
        for a, b in zip(with_field, fresh(theta)):
            assert np.array_equal(a, b)
        for a, b in zip(without, fresh(None)):
            assert np.array_equal(a, b)
        for a, b in zip(again, with_field):
            assert np.array_equal(a, b)
        assert not np.array_equal(with_field[0], without[0])
        if model == "NEO_HOOKEAN":   # the tangent, its Dirichlet scale and the stable step see the field; linear elasticity's do not
            assert not np.array_equal(with_field[1], without[1]) and not np.array_equal(with_field[3], without[3])
        else:
            assert np.array_equal(with_field[1], without[1]) and np.array_equal(with_field[3], without[3])
        # a mesh change drops the field
        eng.set_element_expansion(theta)
        asm2 = assembler(eng, m, model, w, p, u_mid)
        with pytest.raises(fa.FenrisError) as ei:
            eng.element_expansion()
        assert ei.value.code == FH_INVALID_STATE
        eng2 = fa.Engine(0)
        try:
            assert np.array_equal(fa.VectorAssembler().assemble_vector(asm2), fa.VectorAssembler().assemble_vector(assembler(eng2, m, model, w, p, u_mid)))
        finally:
            eng2.close()
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------ 10. refusals, arguments
def _raises(code, fn, *words):
    with pytest.raises(fa.FenrisError) as ei:
        fn()
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    for wd in words:
        assert wd in str(ei.value), str(ei.value)


@pytest.mark.gpu
def test_arguments(engine):
    m, w, p = small_mesh("HEX8")
    E, n = m.num_elements(), 3 * m.num_nodes()
    lib, h = engine._lib, engine._h
    one = np.ones(E + 1)
    assert lib.fh_set_element_expansion(h, _ffi.fp(one), 1) == FH_INVALID_STATE   # no mesh yet
    asm = assembler(engine, m, "LINEAR_ELASTIC", w, p, np.zeros(n))
    _raises(FH_INVALID_STATE, engine.element_expansion, "expansion")
    assert lib.fh_set_element_expansion(h, _ffi.fp(one), 2) == FH_BAD_ARGUMENT
    assert lib.fh_set_element_expansion(h, _ffi.fp(one), E + 1) == FH_BAD_ARGUMENT
    good = random_theta(m)
    engine.set_element_expansion(good)
    for bad_value in (0.0, -1.0, np.nan, np.inf):
        th = good.copy()
        th[5], th[6] = bad_value, bad_value
        _raises(FH_BAD_ARGUMENT, lambda: engine.set_element_expansion(th), "element 5")
        assert np.array_equal(engine.element_expansion(), good)   # the standing field is kept
    _raises(FH_BAD_ARGUMENT, lambda: engine.set_element_expansion(-2.0), "element 0")
    # a temperature that drives theta non-positive: the lowest element is named
    T = np.zeros(m.num_nodes())
    alpha = np.full(E, 1e-3)
    alpha[3], alpha[6] = 1.0, 1.0
    T[:] = -2.0
    _raises(FH_BAD_ARGUMENT, lambda: engine.set_thermal_expansion(T, alpha, 0.0), "element 3")
    assert np.array_equal(engine.element_expansion(), good)
    _raises(FH_BAD_ARGUMENT, lambda: engine.set_thermal_expansion(T, alpha[:3], 0.0), "alpha_count")
    T[0] = np.nan
    _raises(FH_BAD_ARGUMENT, lambda: engine.set_thermal_expansion(T, 1e-3, 0.0), "element")
    # clearing: None, and a count of zero
    engine.set_element_expansion(None)
    _raises(FH_INVALID_STATE, engine.element_expansion)
    engine.set_element_expansion(good)
    assert lib.fh_set_element_expansion(h, _ffi.fp(good), 0) == 0
    _raises(FH_INVALID_STATE, engine.element_expansion)
    _raises(FH_INVALID_STATE, engine.thermal_load, "expansion")
    # the device entry points
    import torch

    td = torch.tensor(good, device="cuda:0")
    assert lib.fh_set_element_expansion_dev(h, C.c_void_p(td.data_ptr()), E) == 0
    assert np.array_equal(engine.element_expansion(), good)
    Td, ad = torch.full((m.num_nodes(),), 30.0, dtype=torch.float64, device="cuda:0"), torch.tensor([1e-4], dtype=torch.float64, device="cuda:0")
    assert lib.fh_set_thermal_expansion_dev(h, C.c_void_p(Td.data_ptr()), C.c_void_p(ad.data_ptr()), 1, 10.0) == 0
    assert np.abs(engine.element_expansion() - (1.0 + 1e-4 * 20.0)).max() <= 4e-16
    del asm


@pytest.mark.gpu
def test_refusals_name_the_expansion(engine):
    import torch

    m, w, p = small_mesh("HEX8")
    E, N = m.num_elements(), m.num_nodes()
    theta = random_theta(m)
    clamp = np.where(m.vertices[:, 0] < 0.1)[0]
    # FH_LAPLACE on every route
    qt = fa.UniformQuadratureTable.from_points_and_weights(p, w)
    lap = (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(m).with_operator(fa.LaplaceOperator()).with_quadrature_table(qt)
           .with_u(np.zeros(N)).build())
    engine.set_element_expansion(theta)
    x = np.ones(N)
    routes = [lambda: fa.VectorAssembler().assemble_vector(lap), lambda: fa.assemble_scalar(lap),
              lambda: fa.MatrixFreeTangent(lap).apply(np.zeros(N), x), lambda: fa.MatrixFreeTangent(lap).diagonal(),
              lambda: fa.MatrixFreeShiftedTangent(lap, 1.0, 1.0, 1.0).apply(np.zeros(N), x),
              lambda: fa.MatrixFreeNewton(lap).with_dirichlet_nodes(clamp).solve(np.zeros(N), fa.NewtonSettings(3, 1e-8)),
              lambda: fa.ThetaMethod(lap, 1.0, 1e-3).with_dirichlet_nodes(clamp).set_state(np.zeros(N)).step(1),
              lambda: fa.MatrixFreeEigensolver(lap, 1.0).with_dirichlet_nodes(clamp).solve(2),
              lambda: engine.recover("grad_u", "points"), engine.thermal_load]
    for fn in routes:
        _raises(FH_UNSUPPORTED, fn, "expansion")
    fa.CsrAssembler(fa.SCATTER_GATHER).assemble(lap)   # (no elastic strain in that matrix: allowed)
    engine.set_element_expansion(None)
    fa.VectorAssembler().assemble_vector(lap)
    # FH_TENSOR
    tens = np.einsum("ik,jl->ijkl", np.eye(3), np.eye(3))
    ten = (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(m).with_operator(fa.TensorEllipticOperator(tens, True))
           .with_quadrature_table(qt).with_u(np.zeros(3 * N)).build())
    engine.set_element_expansion(theta)
    _raises(FH_UNSUPPORTED, lambda: fa.MatrixFreeTangent(ten).apply(np.zeros(3 * N), np.ones(3 * N)), "expansion")
    fa.CsrAssembler(fa.SCATTER_GATHER).assemble(ten)
    # the assembled stiffness: hyperelastic refused, linear elasticity and the mass allowed and unchanged
    for model in ("NEO_HOOKEAN", "STVK", "STABLE_NEO_HOOKEAN"):
        asm = assembler(engine, m, model, w, p, np.zeros(3 * N))
        engine.set_element_expansion(theta)
        _raises(FH_UNSUPPORTED, lambda: fa.CsrAssembler(fa.SCATTER_GATHER).assemble(asm), "expansion")
        _raises(FH_UNSUPPORTED, lambda: engine.element_matrices(0, 1), "expansion")
        _raises(FH_UNSUPPORTED, engine.thermal_load, "expansion")
        fa.VectorAssembler().assemble_vector(asm)
    asm = assembler(engine, m, "LINEAR_ELASTIC", w, p, np.zeros(3 * N))
    k0 = fa.CsrAssembler(fa.SCATTER_GATHER).assemble(asm).values
    engine.set_element_expansion(theta)
    k1 = fa.CsrAssembler(fa.SCATTER_GATHER).assemble(asm).values
    assert np.array_equal(np.asarray(k0.cpu() if hasattr(k0, "cpu") else k0), np.asarray(k1.cpu() if hasattr(k1, "cpu") else k1))


@pytest.mark.gpu
def test_multigrid_and_rule_sets_and_ragged_connectivity(engine):
    # FH_PRECOND_MULTIGRID: refused with a hyperelastic operator, allowed (and the solve of the Jacobi-preconditioned one) with linear elasticity
    meshes, ts = fa.refine_uniformly_repeat_with_transfers(fa.procedural.create_unit_box_uniform_hex_mesh_3d(2), 1)
    fine = meshes[-1]
    w, p = map(np.asarray, quadrature.tensor.hexahedron_gauss(2))
    nf = 3 * fine.num_nodes()
    clamp = np.where(fine.vertices[:, 0] < 1e-9)[0]
    theta_f = random_theta(fine, lo=0.99, hi=1.01)
    for model in ("NEO_HOOKEAN", "STVK", "STABLE_NEO_HOOKEAN"):
        asm = assembler(engine, fine, model, w, p, np.zeros(nf))
        mg = fa.GeometricMultigrid(asm, meshes[:-1], ts)
        engine.set_element_expansion(theta_f)
        solver = fa.MatrixFreeNewton(asm).with_dirichlet_nodes(clamp).with_multigrid(mg)
        _raises(FH_UNSUPPORTED, lambda: solver.solve(np.zeros(nf), fa.NewtonSettings(5, 1e-6)), "expansion", "MULTIGRID")
        del solver, mg
    asm = assembler(engine, fine, "LINEAR_ELASTIC", w, p, np.zeros(nf))
    mg = fa.GeometricMultigrid(asm, meshes[:-1], ts)
    engine.set_element_expansion(theta_f)
    f_th = engine.thermal_load()
    tol = 1e-8 * np.linalg.norm(f_th)
    u_mg, u_j = np.zeros(nf), np.zeros(nf)
    fa.MatrixFreeNewton(asm).with_dirichlet_nodes(clamp).with_multigrid(mg).solve(u_mg, fa.NewtonSettings(20, tol), linear_rel_tol=1e-12)
    asm.with_u(np.zeros(nf))
    fa.MatrixFreeNewton(asm).with_dirichlet_nodes(clamp).solve(u_j, fa.NewtonSettings(20, tol), preconditioner=fa.PRECOND_JACOBI, linear_rel_tol=1e-12)
    assert np.abs(u_j).max() > 0.0 and np.abs(u_mg - u_j).max() <= 1e-8 * np.abs(u_j).max()
    del mg
    # rule-set tables
    m, w, p = small_mesh("HEX8")
    E, N = m.num_elements(), m.num_nodes()
    w3, p3 = map(np.asarray, quadrature.tensor.hexahedron_gauss(3))
    qt = fa.GeneralQuadratureTable.from_points_weights_and_data([(p, p3)[e % 2] for e in range(E)], [(w, w3)[e % 2] for e in range(E)],
                                                                 [[LAME] * len((w, w3)[e % 2]) for e in range(E)])
    asm = (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(m).with_operator(fa.MaterialEllipticOperator(fa.StVKMaterial()))
           .with_quadrature_table(qt).with_u(np.zeros(3 * N)).build())
    engine.set_element_expansion(1.05)
    _raises(FH_UNSUPPORTED, lambda: fa.VectorAssembler().assemble_vector(asm), "expansion")
    _raises(FH_UNSUPPORTED, lambda: fa.assemble_scalar(asm), "expansion")
    _raises(FH_UNSUPPORTED, lambda: fa.MatrixFreeTangent(asm).apply(np.zeros(3 * N), np.ones(3 * N)), "expansion")
    engine.set_element_expansion(None)
    fa.VectorAssembler().assemble_vector(asm)
    # ragged connectivity: the setter refuses, and setting it drops a standing field
    lib, h = engine._lib, engine._h
    assembler(engine, m, "STVK", w, p, np.zeros(3 * N))
    engine.set_element_expansion(1.05)
    eoff = np.arange(0, 8 * E + 1, 8, dtype=np.uint64)
    nodes = np.ascontiguousarray(m.connectivity, dtype=np.uint64).reshape(-1)
    assert lib.fh_set_connectivity_ragged(h, 3, N, _ffi.up(eoff), _ffi.up(nodes), E) == 0
    one = np.ones(1)
    assert lib.fh_set_element_expansion(h, _ffi.fp(one), 1) == FH_UNSUPPORTED and "expansion" in engine.last_error()
    assert lib.fh_element_expansion(h, _ffi.fp(np.zeros(E))) == FH_INVALID_STATE
