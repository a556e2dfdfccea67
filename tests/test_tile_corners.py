"""Every tile kernel and node pass of fenris_amd/csrc/vector_tiles.hip at the corners of the tile tables, against the long-double reference
(hp_reference.py): scattered tiles with more than 512 distinct nodes, nodes with 5 .. 11 partials, nodes without elements, the node count
against the 256 threads of a node pass's workgroup, the tile count against the eight shares of the element pass's grid.

The meshes (tile_tables_model.corner_cases) are valid geometry on tiles the model predicts: a dealt mesh is handed over with every vertex at
the origin (all Morton keys equal: tile t is the elements [256 t, 256 t + 256)), its tables are built by the stats call, and
fh_update_vertices, which keeps the tables, gives it its coordinates.  Every test first checks that the device's tables are the model's, so a
test that passes did run on the corner it names.

Bars: 1e-12 x the rounding scale of the quantity, taken from the reference (|| (|alpha| |M| + |beta| |K|) |x| ||_inf for a map, max |d| for
a diagonal, the propagated scale for a scalar); the largest error / bar per route and mesh is printed at the end of the module."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import fenris_amd as fa
import hp_reference as hp
import stable_neo_hookean_reference as snh
import tile_tables_model as ttm
from fenris_amd import _ffi, quadrature

pytestmark = pytest.mark.gpu
LD = np.longdouble
LAME = fa.LameParameters(3.0e2, 5.0e2)
RULES = {"HEX8": quadrature.tensor.hexahedron_gauss(2), "TET4": quadrature.total_order.tetrahedron(2),
         "QUAD4": quadrature.tensor.quadrilateral_gauss(2), "TRI3": quadrature.total_order.triangle(2)}
MATERIALS = {"LINEAR_ELASTIC": fa.LinearElasticMaterial, "NEO_HOOKEAN": fa.NeoHookeanMaterial, "STVK": fa.StVKMaterial,
             "STABLE_NEO_HOOKEAN": fa.StableNeoHookeanMaterial}
LINEAR = ("LAPLACE", "LINEAR_ELASTIC")
CASES = list(ttm.corner_cases())
SNH_CASES = ("hex8 dealt", "hex8 dealt affine", "tet4 dealt")
COMBOS = [(c, m) for c in CASES for m in ("LAPLACE", "LINEAR_ELASTIC", "NEO_HOOKEAN", "STVK") + (("STABLE_NEO_HOOKEAN",) if c in SNH_CASES else ())]
DIAG_ROUTE, MASS_DIAG_ROUTE, MASS_ROUTE = ("k_diagonal_tiled + k_vector_from_partials", "k_mass_tiled + k_vector_from_partials",
                                           "k_mass_tiled + k_shift_from_partials")
ELEMENT_ROUTE = {True: "k_element_pass_tiled + k_operator_from_partials", False: "k_tangent_tiled + k_operator_from_partials"}
MARGINS = {}


def _le(key, err, bar):
    """records error / bar under its key and asserts"""
    err, bar = float(err), float(bar)
    assert np.isfinite(err) and bar > 0.0, (key, err, bar)
    MARGINS[key] = max(MARGINS.get(key, 0.0), err / bar)
    print(f"{key}: error {err:.3e} bar {bar:.3e} ratio {err / bar:.3f}")
    assert err <= bar, (key, err, bar)


@pytest.fixture(scope="module", autouse=True)
def _print_margins():
    yield
    if MARGINS:
        print("\nlargest error / bar per route and mesh:")
        for k in sorted(MARGINS):
            print(f"  {k:110s} {MARGINS[k]:.3f}")


@pytest.fixture()
def engine():
    eng = fa.Engine(0)
    yield eng
    eng.close()


def _engine_without_tiles():
    os.environ["FENRIS_HIP_NO_VECTOR_TILES"] = "1"
    try:
        return fa.Engine(0)
    finally:
        del os.environ["FENRIS_HIP_NO_VECTOR_TILES"]


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")


# ---- the problems: mesh, smooth u with det F > 0, element densities, Dirichlet set, element mask, and the references, built once
_PROBLEMS, _REFS = {}, {}


def _smooth_u(X, s, amp):
    lo, hi = X.min(axis=0), X.max(axis=0)
    L = float((hi - lo).max())
    xi = (X - lo) / L
    u = np.zeros((len(X), s))
    for k in range(s):
        a = np.cos(1.0 + np.arange(3) + 2.0 * k)
        u[:, k] = amp * L * (a[0] * np.sin(np.pi * xi[:, 0]) * np.cos(0.5 * np.pi * xi[:, 1]) + a[1] * np.sin(np.pi * xi[:, 1])
                             + a[2] * np.cos(np.pi * xi.sum(axis=1)))
    return u.reshape(-1)


def problem(case_name, model):
    key = (case_name, model)
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    case = ttm.corner_cases()[case_name]
    mesh = case.mesh
    d = mesh.vertices.shape[1]
    s = 1 if model == "LAPLACE" else d
    rng = np.random.default_rng(1000 * CASES.index(case_name) + len(model))
    E, N = mesh.num_elements(), mesh.num_nodes()
    conn = np.asarray(mesh.connectivity).astype(np.int64)
    unused = ttm.unused_nodes(mesh)
    used = np.setdiff1d(np.arange(N), unused)
    face = used[mesh.vertices[used, 0] < mesh.vertices[used, 0].min() + 0.5]
    mask = (rng.random(E) < 0.6).astype(np.uint8)
    only_inactive = np.setdiff1d(conn[mask == 0].reshape(-1), conn[mask == 1].reshape(-1))
    p = SimpleNamespace(case=case, mesh=mesh, kind=case.kind, model=model, d=d, s=s, n=s * N, E=E, N=N, conn=conn, unused=unused,
                        dirichlet=np.union1d(unused, face), u=_smooth_u(mesh.vertices, s, 0.04), rho=1.0 + rng.random(E), mask=mask,
                        only_inactive=only_inactive, rule=tuple(np.asarray(a) for a in RULES[case.kind]),
                        lame=LAME.for_stable_neo_hookean(d) if model == "STABLE_NEO_HOOKEAN" else LAME)
    p.fixed = np.zeros(p.n, dtype=bool)
    p.fixed.reshape(N, s)[p.dirichlet] = True
    p.unused_dofs = np.zeros(p.n, dtype=bool)
    p.unused_dofs.reshape(N, s)[unused] = True
    _PROBLEMS[key] = p
    return p


def reference(p, masked=False, rho=None):
    """the long-double reference of the problem at its u (masked: of the active elements alone, at the u with a huge value on the nodes
    that only inactive elements touch for the hyperelastic models; rho: one density for the mesh instead of the problem's element
    densities), built once per (mesh, model, variant)"""
    key = (p.case.name, p.model, masked, rho)
    if key not in _REFS:
        w, pts = p.rule
        conn, rho, u = (p.conn[p.mask == 1], p.rho[p.mask == 1], masked_u(p)) if masked else (p.conn, p.rho if rho is None else rho, p.u)
        if p.model == "STABLE_NEO_HOOKEAN":
            ref = snh.Reference(p.kind, p.mesh.vertices, conn, w, pts, u, p.lame.mu, p.lame.lambda_, rho=rho)
        else:
            ref = hp.Reference(p.kind, p.model, p.mesh.vertices, conn, w, pts, u, p.lame.mu, p.lame.lambda_, rho=rho)
            if p.model in ("NEO_HOOKEAN", "STVK"):
                assert ref.det_F_min > 0.2, ref.det_F_min
        _REFS[key] = ref
    return _REFS[key]


def masked_u(p):
    um = p.u.copy()
    if p.model not in LINEAR:
        rng = np.random.default_rng(9)
        um.reshape(p.N, p.s)[p.only_inactive] = 50.0 * rng.standard_normal((len(p.only_inactive), p.s))
    return um


def bind(engine, p, u=None, check_tables=True):
    """the assembler of the problem on this engine, on the tiles the model predicts (see the module's docstring)"""
    w, pts = p.rule
    qt = fa.UniformQuadratureTable.from_points_and_weights(pts, w)
    op = fa.LaplaceOperator() if p.model == "LAPLACE" else fa.MaterialEllipticOperator(MATERIALS[p.model]())
    if p.model != "LAPLACE":
        qt = qt.with_uniform_data(p.lame)
    first = ttm.collapsed(p.mesh) if p.case.dealt else p.mesh
    asm = (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(first).with_operator(op).with_quadrature_table(qt)
           .with_u(p.u if u is None else u).build())
    got = engine.vector_tiles_stats()          # (builds the tables: with the vertices that are set now)
    if p.case.dealt:
        engine.update_vertices(p.mesh.vertices)
        assert engine.vector_tiles_stats() == got            # the tables survive the update
    if check_tables:
        if p.case.model is not None:
            assert got == ttm.stats(p.case.model), (p.case.name, got)
        else:
            assert got[0] == p.case.natural_tiles and got[1] <= p.E * p.conn.shape[1], (p.case.name, got)
    return asm


def _map(asm, p):
    return fa.MatrixFreeOperator(asm) if p.model in LINEAR else fa.MatrixFreeTangent(asm)


def _apply_twice(op, x):
    """y = op x from a y full of NaN, twice: the same bits"""
    import torch

    xt = _dev(x)
    y1 = torch.full_like(xt, float("nan"))
    op.apply(y1, xt)
    name = op.engine.last_kernel_name()
    y2 = torch.full_like(xt, float("nan"))
    op.apply(y2, xt)
    a, b = _host(y1), _host(y2)
    assert np.array_equal(a, b) and np.all(np.isfinite(a))
    return a, name


def _diagonal(op, alpha=0.0):
    """the map's diagonal, twice for equal bits, with the route of its last element pass: k_diagonal_tiled, or with a mass term (formed
    after the stiffness term) k_mass_tiled in its diagonal form"""
    d = op.diagonal()
    name = op.engine.last_kernel_name()
    assert name == (MASS_DIAG_ROUTE if alpha else DIAG_ROUTE), name
    assert np.array_equal(d, op.diagonal())
    return d


def _first_nonzero(d):
    nz = np.nonzero(np.asarray(d, dtype=np.float64))[0]
    return abs(float(d[nz[0]])) if len(nz) else 1.0


def _check_dirichlet_apply(tag, p, op, ref, x, alpha, beta, want_route):
    """the map with the problem's Dirichlet set (every node without elements and one face): free rows against the reference of x with
    the constrained entries zero, constrained rows  scale x  exactly, scale the one value the diagonal holds there"""
    op.with_dirichlet_nodes(p.dirichlet)
    diag = _diagonal(op, alpha)
    scale = diag[p.fixed]
    assert np.all(scale == scale[0]) and scale[0] > 0.0
    scale = scale[0]
    dref = (alpha * ref.diagonal("M") if alpha else 0) + (beta * ref.diagonal("K") if beta else 0)
    assert abs(scale - _first_nonzero(dref)) <= 1e-12 * scale, (tag, scale)
    y, name = _apply_twice(op, x)
    assert name == want_route, (tag, name, want_route)
    x0 = np.where(p.fixed, 0.0, x)
    want, _ = ref.apply(x0, alpha, beta)
    rows = ref.abs_apply(x0, alpha, beta)
    _le(tag, np.abs(y - want)[~p.fixed].max(), 1e-12 * float(rows.max()))
    assert np.array_equal(y[p.fixed], scale * x[p.fixed]), tag
    op.with_dirichlet_nodes(None)
    return y


# ---- (0) the device's tables are the model's, on every mesh
@pytest.mark.parametrize("name", CASES)
def test_tables_equal_the_model(engine, name):
    p = problem(name, "LAPLACE")
    bind(engine, p)
    t, parts, mt, mp = engine.vector_tiles_stats()
    assert t == p.case.natural_tiles and parts <= p.E * p.conn.shape[1] and 0 < mt <= 256 * p.conn.shape[1] and mp >= 1
    if p.case.model is not None:
        assert (t, parts, mt, mp) == ttm.stats(p.case.model)
    # a mesh without tiles: FH_UNSUPPORTED
    eng2 = _engine_without_tiles()
    try:
        bind_off = fa.ElementEllipticAssemblerBuilder(eng2).with_finite_element_space(p.mesh).with_operator(fa.LaplaceOperator()) \
            .with_quadrature_table(fa.UniformQuadratureTable.from_points_and_weights(p.rule[1], p.rule[0])).with_u(p.u).build()
        with pytest.raises(fa.FenrisError) as ei:
            bind_off.engine.vector_tiles_stats()
        assert ei.value.code == _ffi.FH_UNSUPPORTED
    finally:
        eng2.close()


# ---- (a) the operator / tangent apply, (b) the diagonals
@pytest.mark.parametrize("name,model", COMBOS)
def test_operator_apply_and_diagonal(engine, name, model):
    p = problem(name, model)
    ref = reference(p)
    asm = bind(engine, p)
    op = _map(asm, p)
    rng = np.random.default_rng(31)
    x = rng.standard_normal(p.n)
    route = ELEMENT_ROUTE[model in LINEAR]
    tag = f"{route} | {model} | {name}"
    y, got_route = _apply_twice(op, x)
    assert got_route == route, got_route
    want, bound = ref.apply(x)
    _le(tag, np.abs(y - want).max(), 1e-12 * bound)
    assert not np.any(y[p.unused_dofs])      # rows of nodes without elements: exactly 0.0
    # the diagonal (k_diagonal_tiled: the linear and the tangent form)
    d = _diagonal(op)
    dref = ref.diagonal()
    _le(f"{DIAG_ROUTE} | {model} | {name}", np.abs(d - dref).max(), 1e-12 * float(np.abs(dref).max()))
    assert not np.any(d[p.unused_dofs])
    # Dirichlet rows; then constrained entries 1e15 times the free ones (LinearElastic: the operand's exponent comes from the free entries)
    _check_dirichlet_apply(tag + " | dirichlet", p, op, ref, x, 0.0, 1.0, route)
    big = np.where(p.fixed, 1e12, 1e-3) * x
    _check_dirichlet_apply(tag + " | dirichlet 1e15", p, op, ref, big, 0.0, 1.0, route)


@pytest.mark.parametrize("mono", [0, 1, 2])
@pytest.mark.parametrize("model", ["NEO_HOOKEAN", "LINEAR_ELASTIC"])
def test_hex8_forms_of_the_element_pass(engine, mono, model):
    """Hex8: the general form (the monomial table switched off), the monomial form on distorted elements, the affine form (LinearElastic:
    with the rule's moments) -- the tangent and the residual's element pass fed the operand, on scattered tiles"""
    name = "hex8 dealt affine" if mono == 2 else "hex8 dealt"
    if mono == 0:
        engine.set_option("FENRIS_HIP_NO_MONOMIAL", "1")
    p = problem(name, model)
    ref = reference(p)
    op = _map(bind(engine, p), p)
    # what selects the form: every element classified affine after the vertex update (or none), at the default tolerance
    assert engine.affine_stats()[0] == (p.E if mono == 2 else 0)
    x = np.random.default_rng(32).standard_normal(p.n)
    y, route = _apply_twice(op, x)
    assert route == ELEMENT_ROUTE[model in LINEAR]
    want, bound = ref.apply(x)
    _le(f"{route} | {model} | {name} | form {mono}", np.abs(y - want).max(), 1e-12 * bound)
    # the forms are different arithmetic: on the same mesh, with the next form switched off, the bits differ and the bar still holds
    other = fa.Engine(0)
    try:
        other.set_option({0: "FENRIS_HIP_NO_AFFINE_PASS", 1: "FENRIS_HIP_NO_MONOMIAL", 2: "FENRIS_HIP_NO_AFFINE_PASS"}[mono], "1")
        if mono == 0:
            other.set_option("FENRIS_HIP_NO_MONOMIAL", "1")      # (distorted elements: the affine switch changes nothing, the same bits)
        y2, _ = _apply_twice(_map(bind(other, p), p), x)
    finally:
        other.close()
    # (the all-affine tangent only drops the mixed coefficients of the geometry map, which are exactly zero on these cubes: the same bits
    # as the monomial form, so there the affine count above is what shows the form; LinearElastic takes the rule's moments instead)
    if mono != 2 or model in LINEAR:
        assert np.array_equal(y, y2) == (mono == 0), mono
    _le(f"{route} | {model} | {name} | form {mono}, neighbouring form", np.abs(y2 - want).max(), 1e-12 * bound)


# ---- (c) the mass: apply, diagonal, lumped
def _mass_combos():
    return [(c, m) for c in CASES for m in ("LAPLACE", "LINEAR_ELASTIC")]


@pytest.mark.parametrize("per_element", [False, True])
@pytest.mark.parametrize("name,model", _mass_combos())
def test_mass_apply_diagonal_and_lumped(engine, name, model, per_element):
    p = problem(name, model)
    rho = p.rho if per_element else 1.75
    ref = reference(p) if per_element else reference(p, rho=rho)
    hex_fused = p.kind == "HEX8"
    for no_mono in ((0, 1) if hex_fused else (0,)):
        eng = engine if not no_mono else fa.Engine(0)
        try:
            if no_mono:
                eng.set_option("FENRIS_HIP_NO_MONOMIAL", "1")
            asm = bind(eng, p)
            mass = fa.MatrixFreeMass(asm, rho)
            x = np.random.default_rng(33).standard_normal(p.n)
            y, route = _apply_twice(mass, x)
            fused = hex_fused and not no_mono
            label = "k_mass_hex8_tiled + k_operator_from_partials" if fused else MASS_ROUTE
            assert route == label, route
            tag = f"{label} | S={p.s} rho/{'element' if per_element else 'mesh'} | {name}"
            want, bound = ref.apply(x, 1.0, 0.0)
            _le(tag, np.abs(y - want).max(), 1e-12 * bound)
            assert not np.any(y[p.unused_dofs])
            d = _diagonal(mass, 1.0)
            dref = ref.diagonal("M")
            _le(tag + " | diagonal", np.abs(d - dref).max(), 1e-12 * float(np.abs(dref).max()))
            lumped = mass.lumped()
            assert eng.last_kernel_name() == label, eng.last_kernel_name()
            ones = np.ones(p.n)
            want1, bound1 = ref.apply(ones, 1.0, 0.0)
            _le(tag + " | lumped", np.abs(lumped - want1).max(), 1e-12 * bound1)
            assert not np.any(lumped[p.unused_dofs])
            # the operand with the Dirichlet entries read as zero, the rows  scale x
            _check_dirichlet_apply(tag + " | dirichlet", p, mass, ref, x, 1.0, 0.0, label)
        finally:
            if no_mono:
                eng.close()


# ---- (d) the shifted map alpha M + beta T(u)
@pytest.mark.parametrize("name,model", COMBOS)
def test_shifted_map(engine, name, model):
    p = problem(name, model)
    ref = reference(p)
    asm = bind(engine, p)
    x = np.random.default_rng(34).standard_normal(p.n)
    linear = model in LINEAR
    for alpha, beta in ((1.0, 1e-4), (2.0, 0.0), (0.0, 3.0)):
        sh = fa.MatrixFreeShiftedTangent(asm, p.rho, alpha, beta)
        y, route = _apply_twice(sh, x)
        if p.kind == "HEX8" and alpha != 0.0:
            want_route = ("k_mass_hex8_tiled" if beta == 0.0 else "k_shifted_pass_tiled" if linear else "k_shifted_tangent_tiled") + " + k_operator_from_partials"
            label = want_route
        else:   # the tangent's pass, whose name stays, then (alpha != 0) k_mass_tiled and the shift node pass, named where they run alone:
            # whether the mass pass takes the tiles does not depend on beta (mass_tiles_pass), so the (2, 0) pair speaks for (1, 1e-4) too
            want_route = ELEMENT_ROUTE[linear] if beta != 0.0 else MASS_ROUTE
            label = ELEMENT_ROUTE[linear] if alpha == 0.0 else (MASS_ROUTE if beta == 0.0
                                                                else ELEMENT_ROUTE[linear].split(" + ")[0] + " + k_mass_tiled + k_shift_from_partials")
        assert route == want_route, (route, want_route)
        tag = f"{label} | {model} ({alpha:g}, {beta:g}) | {name}"
        want, bound = ref.apply(x, alpha, beta)
        _le(tag, np.abs(y - want).max(), 1e-12 * bound)
        assert not np.any(y[p.unused_dofs])
        _check_dirichlet_apply(tag + " | dirichlet", p, sh, ref, x, alpha, beta, want_route)
        d = _diagonal(sh, alpha)
        dref = (alpha * ref.diagonal("M") if alpha else 0) + (beta * ref.diagonal("K") if beta else 0)
        _le(tag + " | diagonal", np.abs(d - dref).max(), 1e-12 * float(np.abs(dref).max()))


# ---- (e) the per-workgroup partials of x . y: one PCG iteration hands back x_1 = (b . b) / (b . A b) b
PCG_CASES = ["hex8 soup N=1", "hex8 soup N=0", "tet4 soup N=1", "tet4 soup N=0", "hex8 dealt", "tet4 dealt", "tri3 dealt", "quad4 first 257"]


@pytest.mark.parametrize("entry", ["matrix_free", "tangent", "shifted_tangent"])
@pytest.mark.parametrize("name", PCG_CASES)
def test_one_pcg_iteration_returns_the_first_iterate(engine, name, entry):
    import torch

    model = {"matrix_free": "LINEAR_ELASTIC", "tangent": "NEO_HOOKEAN", "shifted_tangent": "NEO_HOOKEAN"}[entry]
    p = problem(name, model)
    ref = reference(p)
    asm = bind(engine, p)
    alpha, beta = (1.0, 1e-2) if entry == "shifted_tangent" else (0.0, 1.0)
    op = {"matrix_free": fa.MatrixFreeOperator, "tangent": fa.MatrixFreeTangent}.get(entry, lambda a: fa.MatrixFreeShiftedTangent(a, p.rho, alpha, beta))(asm)
    op.with_dirichlet_nodes(p.dirichlet)         # (every node without elements is held: its row is  scale x, and joins the dot product)
    b = np.random.default_rng(35).standard_normal(p.n)
    got = []
    for _ in range(2):
        x = torch.zeros(p.n, dtype=torch.float64, device="cuda:0")
        with pytest.raises(fa.CgSolveError) as ei:
            op.cg_solve(_dev(b), x, preconditioner=_ffi.PRECOND_IDENTITY, rel_tol=1e-30, max_iter=1)
        assert ei.value.code == _ffi.FH_CG_MAX_ITERATIONS and ei.value.num_iterations == 1
        got.append(_host(x))
    route = engine.last_kernel_name()
    want_route = ("k_shifted_tangent_tiled + k_operator_from_partials" if p.kind == "HEX8" else ELEMENT_ROUTE[False]) if entry == "shifted_tangent" \
        else ELEMENT_ROUTE[model in LINEAR]
    assert route == want_route, route
    assert np.array_equal(got[0], got[1])
    # A with the Dirichlet rows: free rows (alpha M + beta K) b0 with b0 = b zeroed on the set, rows of the set  scale b
    dref = (alpha * ref.diagonal("M") if alpha else 0) + beta * ref.diagonal("K")
    scale = LD(_first_nonzero(dref))
    bl = b.astype(LD)
    b0 = np.where(p.fixed, LD(0), bl)
    Ab, _ = ref.apply(b0, alpha, beta)
    Ab = np.where(p.fixed, scale * bl, Ab)
    absAb = np.where(p.fixed, scale * np.abs(bl), ref.abs_apply(b0, alpha, beta))
    bAb = np.sum(bl * Ab)
    x1 = np.sum(bl * bl) / bAb * bl
    bar = 1e-12 * float(np.sum(np.abs(bl) * absAb) / bAb) * float(np.abs(x1).max())
    _le(f"fh_cg_solve_{entry}_dev: x . y partials | {model} | {name}", np.abs(got[0] - x1).max(), bar)


# ---- (f) the Newton node pass
@pytest.mark.parametrize("name,model", COMBOS)
def test_newton_residual_norm(engine, name, model):
    p = problem(name, model)
    ref = reference(p)
    asm = bind(engine, p)
    rng = np.random.default_rng(36)
    f = 0.3 * float(np.abs(ref.residual()).max()) * rng.standard_normal(p.n)
    u_ref = p.u + 0.01 * float(np.abs(p.u).max()) * rng.standard_normal(p.n)
    r = ref.residual()
    rscale = ref.residual_scale()
    dvec = (p.u - u_ref).astype(LD)
    Md, _ = ref.apply(dvec, 1.0, 0.0)
    absMd = ref.abs_apply(dvec, 1.0, 0.0)
    for alpha, beta in ((0.0, 1.0), (1.0, 1e-2)):
        solver = fa.MatrixFreeNewton(asm).with_dirichlet_nodes(p.dirichlet).with_load(f)
        if alpha != 0.0:
            solver.with_inertia(p.rho, alpha, beta, u_ref)
        want_route = "k_element_pass_tiled + k_mass_tiled + k_newton_from_partials" if alpha != 0.0 else "k_element_pass_tiled + k_newton_from_partials"
        norms = []
        for _ in range(2):
            u = p.u.copy()
            res = solver.solve(u, fa.NewtonSettings(None, 1e300))        # converged on entry: one evaluation of F and its norm
            assert res.iterations == 0 and res.residual_evaluations == 1 and np.array_equal(u, p.u)
            assert engine.last_kernel_name() == want_route, engine.last_kernel_name()
            norms.append(res.initial_residual_norm)
        assert norms[0] == norms[1]
        F = LD(alpha) * Md + LD(beta) * (r - f.astype(LD))
        F[p.fixed] = 0
        scale = abs(LD(alpha)) * absMd + abs(LD(beta)) * (rscale + np.abs(f).astype(LD))
        scale[p.fixed] = 0
        want = float(np.sqrt(np.sum(F * F)))
        _le(f"{want_route} | {model} ({alpha:g}, {beta:g}) | {name}", abs(norms[0] - want), 1e-12 * float(np.sqrt(np.sum(scale * scale))))


@pytest.mark.parametrize("name,model", COMBOS)
def test_newton_step_agrees_with_the_route_off_the_tiles(engine, name, model):
    """one full Newton step without line search through the fused node pass against the same step with the tiles switched off (the inner
    PCG is capped at 500 iterations, ten times what it takes: its loop has no other way out should a wrong operator hand it NaN)"""
    p = problem(name, model)
    ref = reference(p)
    rng = np.random.default_rng(37)
    f = 0.3 * float(np.abs(ref.residual()).max()) * rng.standard_normal(p.n)
    u_ref = p.u + 0.01 * float(np.abs(p.u).max()) * rng.standard_normal(p.n)
    # (M + beta T(u) has to stay definite for the PCG: for the linear models T is semi-definite and any beta serves; for the others it has
    # to hold on a soup too, whose stressed elements float free -- the reference's element matrices M_e + beta K_e(u) of the Tet4 soup
    # have a negative eigenvalue at beta = 1e-4 for NeoHookean; at 1e-5 the smallest is positive for NeoHookean and StVK)
    alpha, beta = 1.0, (1e-2 if model in LINEAR else 1e-5)
    if name.find("soup") >= 0 and model not in LINEAR:
        assert np.linalg.eigvalsh((ref.me + LD(beta) * ref.ke).astype(np.float64)).min() > 0.0
    eng2 = _engine_without_tiles()
    out = []
    try:
        for eng in (engine, eng2):
            asm = bind(eng, p) if eng is engine else _plain_assembler(eng2, p)
            u = p.u.copy()
            with pytest.raises(fa.MaximumIterationsReached):
                (fa.MatrixFreeNewton(asm).with_dirichlet_nodes(p.dirichlet).with_load(f).with_inertia(p.rho, alpha, beta, u_ref)
                 .solve(u, fa.NewtonSettings(1, 1e-30), line_search=fa.NoLineSearch(), linear_rel_tol=1e-12, linear_max_iter=500))
            out.append(u)
        assert "k_newton_combine" in eng2.last_kernel_name()
    finally:
        eng2.close()
    step = np.abs(out[0] - p.u).max()
    assert step > 0.0
    _le(f"Newton step, tiles against the composed route | {model} | {name}", np.abs(out[0] - out[1]).max(), 1e-9 * step)
    assert np.array_equal(out[0][p.fixed], p.u[p.fixed])


def _plain_assembler(engine, p):
    w, pts = p.rule
    qt = fa.UniformQuadratureTable.from_points_and_weights(pts, w)
    if p.model != "LAPLACE":
        qt = qt.with_uniform_data(p.lame)
    op = fa.LaplaceOperator() if p.model == "LAPLACE" else fa.MaterialEllipticOperator(MATERIALS[p.model]())
    return fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(p.mesh).with_operator(op).with_quadrature_table(qt).with_u(p.u).build()


# ---- (i) an element mask on scattered tiles
MASK_COMBOS = [(c, m) for c in ("hex8 dealt", "tet4 dealt", "quad4 dealt", "tri3 dealt", "hex8 soup N=1") for m in ("NEO_HOOKEAN", "LINEAR_ELASTIC")]


@pytest.mark.parametrize("name,model", MASK_COMBOS)
def test_element_mask_on_scattered_tiles(engine, name, model):
    p = problem(name, model)
    ref = reference(p, masked=True)
    um = masked_u(p)
    if model not in LINEAR and name != "tet4 dealt":      # (tet4 dealt: every node has some twenty elements, none is left to the inactive ones)
        assert len(p.only_inactive) > 0
    asm = bind(engine, p, u=um)
    engine.set_active_elements(p.mask)
    x = np.random.default_rng(38).standard_normal(p.n)
    op = _map(asm, p)
    y, route = _apply_twice(op, x)
    assert route == ELEMENT_ROUTE[model in LINEAR]
    want, bound = ref.apply(x)
    _le(f"{route} | {model} | {name} | 60 % of the elements", np.abs(y - want).max(), 1e-12 * bound)
    d = _diagonal(op)
    dref = ref.diagonal()
    assert np.all(np.isfinite(d))
    _le(f"{DIAG_ROUTE} | {model} | {name} | 60 % of the elements", np.abs(d - dref).max(), 1e-12 * float(np.abs(dref).max()))
    mass = fa.MatrixFreeMass(asm, p.rho)
    ym, mroute = _apply_twice(mass, x)
    assert mroute == ("k_mass_hex8_tiled + k_operator_from_partials" if p.kind == "HEX8" else MASS_ROUTE), mroute
    # (the reference holds the active elements' densities in their order)
    wantm, boundm = ref.apply(x, 1.0, 0.0)
    _le(f"mass apply | S={p.s} | {name} | 60 % of the elements", np.abs(ym - wantm).max(), 1e-12 * boundm)


# ---- (g) the integrators' node passes, (h) the contact term inside the node passes: against the double-precision references of
# test_dynamics.py, test_first_order.py and test_contact.py at their bar -- 20 x what another summation order changes in the reference
# itself, never below 1e-13, relative to the largest magnitude of each quantity
def _rel(x, y):
    return float(np.abs(np.asarray(x) - np.asarray(y)).max() / max(np.abs(np.asarray(y)).max(), 1e-300))


def _oracle_problem(oracle, p, f, perm=None, obstacles=()):
    import contact_reference as cr
    import dynamics_reference as dr

    conn, rho = (p.conn, p.rho) if perm is None else (p.conn[perm], p.rho[perm])
    w, pts = p.rule
    args = (oracle, getattr(oracle, p.kind), getattr(oracle, p.model), p.mesh.vertices, [(conn.astype(np.uint64), w, pts)])
    kw = dict(params=p.lame.as_pair(), rho=[rho], dirichlet=p.dirichlet, f=f)
    return cr.ContactProblem(*args, obstacles=obstacles, **kw) if len(obstacles) else dr.Problem(*args, **kw)


def _step_setup(p):
    rng = np.random.default_rng(39)
    ref = reference(p)
    f = np.where(p.fixed, 0.0, 0.3 * float(np.abs(ref.residual()).max()) * rng.standard_normal(p.n))
    v0 = np.where(p.fixed, 0.0, 0.5 * rng.standard_normal(p.n))
    return f, v0, np.random.default_rng(40).permutation(p.E)


INTEGRATOR_CASES = ["hex8 dealt", "tet4 dealt", "hex8 soup N=1"]


@pytest.mark.parametrize("name", INTEGRATOR_CASES)
def test_central_difference_step_with_a_record(engine, oracle, name):
    import dynamics_reference as dr

    p = problem(name, "NEO_HOOKEAN")
    f, v0, perm = _step_setup(p)
    dt = 5e-3
    runs = [dr.central_difference(_oracle_problem(oracle, p, f, pm), p.u, v0, dt, 1) for pm in (None, perm)]
    d_perm = max(max(_rel(a, b) for a, b in zip(runs[1][:3], runs[0][:3])), max(_rel(runs[1][3][:, c], runs[0][3][:, c]) for c in range(4)))
    tol = max(20.0 * d_perm, 1e-13)
    got = []
    for _ in range(2):
        ti = fa.CentralDifference(bind(engine, p), p.rho, dt).with_dirichlet_nodes(p.dirichlet).with_load(f)
        ti.set_state(p.u, v0)
        ti.state()       # (a_0: the step's launch, named here -- after a record the name is the energy pass's)
        assert engine.last_kernel_name() == "k_element_pass_tiled + k_dynamics_from_partials", engine.last_kernel_name()
        rec = ti.step(1)
        assert engine.last_kernel_name() == "k_element_energy_tiled", engine.last_kernel_name()
        u, v, a, time, step = ti.state()
        ti.close()
        assert step == 1 and rec.steps_done == 1 and len(rec.time) == 1
        got.append((u, v, a, np.stack([rec.kinetic, rec.stored, rec.load_potential, rec.time], axis=1)))
    assert all(np.array_equal(x, y) for x, y in zip(got[0], got[1]))
    for what, x, y in zip(("u", "v", "a"), got[0][:3], runs[0][:3]):
        _le(f"k_element_pass_tiled + k_dynamics_from_partials | {what} | {name}", _rel(x, y), tol)
    for c, what in enumerate(("kinetic", "stored", "load_potential", "time")):
        _le(f"k_element_pass_tiled + k_dynamics_from_partials | {what} | {name}", _rel(got[0][3][:, c], runs[0][3][:, c]), tol)
    assert np.array_equal(got[0][0][p.fixed], p.u[p.fixed]) and not np.any(got[0][1][p.fixed]) and not np.any(got[0][2][p.fixed])


@pytest.mark.parametrize("name", INTEGRATOR_CASES)
def test_runge_kutta_legendre_step_with_a_record(engine, oracle, name):
    import first_order_reference as fr

    p = problem(name, "NEO_HOOKEAN")
    f, _, perm = _step_setup(p)
    dt = 2e-5          # (the rate (f - r) / m is some hundred: a step of a few thousandths of the cell)
    runs = [fr.rkl(_oracle_problem(oracle, p, f, pm), p.u, dt, 3, 1) for pm in (None, perm)]
    d_perm = max(max(_rel(a, b) for a, b in zip(runs[1][:2], runs[0][:2])), max(_rel(runs[1][2][:, c], runs[0][2][:, c]) for c in range(4)))
    tol = max(20.0 * d_perm, 1e-13)
    got = []
    for _ in range(2):
        ti = fa.RungeKuttaLegendre(bind(engine, p), p.rho, dt, stages=3).with_dirichlet_nodes(p.dirichlet).with_load(f)
        ti.set_state(p.u)
        rec = ti.step(1)
        assert engine.last_kernel_name() == "k_element_energy_tiled", engine.last_kernel_name()
        u, rate, time, step = ti.state()     # (the rate of the state: the stage's launch, named here -- the record's energy pass named the step)
        assert engine.last_kernel_name() == "k_element_pass_tiled + k_first_order_from_partials", engine.last_kernel_name()
        ti.close()
        assert step == 1 and rec.steps_done == 1 and len(rec.time) == 1
        got.append((u, rate, np.stack([rec.mass_norm, rec.stored, rec.load_potential, rec.time], axis=1)))
    assert all(np.array_equal(x, y) for x, y in zip(got[0], got[1]))
    for what, x, y in zip(("u", "rate"), got[0][:2], runs[0][:2]):
        _le(f"k_element_pass_tiled + k_first_order_from_partials | {what} | {name}", _rel(x, y), tol)
    for c, what in enumerate(("mass_norm", "stored", "load_potential", "time")):
        _le(f"k_element_pass_tiled + k_first_order_from_partials | {what} | {name}", _rel(got[0][2][:, c], runs[0][2][:, c]), tol)
    assert np.array_equal(got[0][0][p.fixed], p.u[p.fixed])


def test_contact_inside_the_node_passes(engine, oracle):
    """dealt Hex8 with a plane through the body: the shifted map with the contact term (contact_apply in k_operator_from_partials) and the
    Newton residual norm with the contact force"""
    import contact_reference as cr

    name = "hex8 dealt"
    p = problem(name, "NEO_HOOKEAN")
    f, _, perm = _step_setup(p)
    c = 0.5 * (p.mesh.vertices.min(axis=0) + p.mesh.vertices.max(axis=0))
    obs = [("half_space", tuple(c), (1.0, 2.0, 3.0), 2.0e2)]
    assert 0.3 * p.N <= (cr.gap(obs, p.mesh.vertices, p.u) < 0).sum() <= 0.7 * p.N
    obstacles = fa.Obstacles([fa.HalfSpace(tuple(c), (1.0, 2.0, 3.0), 2.0e2)])
    alpha, beta = 1.0, 0.37
    x = np.random.default_rng(41).uniform(-1.0, 1.0, p.n)
    x0 = np.where(p.fixed, 0.0, x)
    refs = []
    for pm in (None, perm):
        prob = _oracle_problem(oracle, p, f, pm, obs)
        A = (alpha * prob.mass() + beta * prob.tangent(p.u)).tocsr()
        F = alpha * (prob.mass() @ (0.1 * x)) + beta * (prob.residual(p.u) - f)
        F[p.fixed] = 0.0
        refs.append((np.asarray(A @ x0).reshape(-1)[~p.fixed], A.diagonal(), np.array([np.linalg.norm(F)])))
    tol = max(20.0 * max(_rel(a, b) for a, b in zip(refs[1], refs[0])), 1e-13)
    asm = bind(engine, p)
    t = fa.MatrixFreeShiftedTangent(asm, p.rho, alpha, beta).with_dirichlet_nodes(p.dirichlet).with_obstacles(obstacles)
    y, route = _apply_twice(t, x)
    assert route == "k_shifted_tangent_tiled + k_operator_from_partials", route
    _le(f"{route} with contact_apply | {name}", _rel(y[~p.fixed], refs[0][0]), tol)
    d = t.diagonal()
    assert np.array_equal(y[p.fixed], d[p.fixed] * x[p.fixed])
    _le(f"shifted diagonal with contact | {name}", _rel(d[~p.fixed], refs[0][1][~p.fixed]), tol)
    y_off, _ = _apply_twice(fa.MatrixFreeShiftedTangent(asm, p.rho, alpha, beta).with_dirichlet_nodes(p.dirichlet).with_obstacles(None), x)
    assert _rel(y_off[~p.fixed], refs[0][0]) > 1e-3                       # (the term is in the map)
    solver = (fa.MatrixFreeNewton(asm).with_dirichlet_nodes(p.dirichlet).with_load(f).with_inertia(p.rho, alpha, beta, p.u - 0.1 * x)
              .with_obstacles(obstacles))
    res = solver.solve(p.u.copy(), fa.NewtonSettings(None, 1e300))
    assert res.iterations == 0 and engine.last_kernel_name() == "k_element_pass_tiled + k_mass_tiled + k_newton_from_partials"
    _le(f"k_newton_from_partials with contact_force | {name}", abs(res.initial_residual_norm - refs[0][2][0]) / refs[0][2][0], tol)


# ---- nodes without elements that no Dirichlet set holds: the tiled routes answer like the routes off the tiles
@pytest.mark.parametrize("name", ["hex8 soup N=1", "tet4 soup N=0", "quad4 first 257"])
def test_unconstrained_nodes_without_elements_agree_with_the_routes_off_the_tiles(engine, name):
    import torch

    p = problem(name, "NEO_HOOKEAN")
    ref = reference(p)
    rng = np.random.default_rng(42)
    f = 0.3 * float(np.abs(ref.residual()).max()) * rng.standard_normal(p.n)
    x = rng.standard_normal(p.n)
    eng2 = _engine_without_tiles()
    out, steps = [], []
    try:
        for eng in (engine, eng2):
            asm = bind(eng, p) if eng is engine else _plain_assembler(eng2, p)
            t = fa.MatrixFreeShiftedTangent(asm, p.rho, 1.0, 1e-5)
            y, _ = _apply_twice(t, x)
            d, lumped = t.diagonal(), fa.MatrixFreeMass(asm, p.rho).lumped()
            res = fa.MatrixFreeNewton(asm).with_load(f).with_inertia(p.rho, 1.0, 1e-4, p.u + 0.01 * x).solve(p.u.copy(), fa.NewtonSettings(None, 1e300))
            assert ("k_newton_from_partials" in eng.last_kernel_name()) == (eng is engine)
            # the x . y partial of a PCG step with free nodes without elements (rows of zeros: b . A b does not see them)
            x1 = torch.zeros(p.n, dtype=torch.float64, device="cuda:0")
            with pytest.raises(fa.CgSolveError):
                t.cg_solve(_dev(x), x1, preconditioner=_ffi.PRECOND_IDENTITY, rel_tol=1e-30, max_iter=1)
            out.append((y, d, lumped, np.array([res.initial_residual_norm]), _host(x1)))
            # the explicit integrators divide by the lumped mass, which is zero there: whatever one route answers, the other answers too
            for make in (lambda: fa.CentralDifference(asm, p.rho, 5e-3), lambda: fa.RungeKuttaLegendre(asm, p.rho, 2e-5, stages=3)):
                ti = make().with_load(f)
                try:
                    ti.set_state(p.u)
                    ti.step(1)
                    state = ti.state()[0]
                    steps.append(("finite", 0) if np.all(np.isfinite(state)) else ("not finite", int(np.isnan(state[p.unused_dofs]).sum())))
                except fa.FenrisError as err:
                    steps.append(("error", err.code))
                finally:
                    ti.close()
    finally:
        eng2.close()
    assert steps[:2] == steps[2:], steps
    for what, a, b in zip(("apply", "diagonal", "lumped mass", "Newton norm", "first PCG iterate"), out[0], out[1]):
        assert np.all(np.isfinite(a)) and np.all(np.isfinite(b)), what
        _le(f"tiles against the routes off the tiles, free nodes without elements | {what} | {name}", _rel(a, b), 1e-12)
    for a in out[0][:3]:
        assert not np.any(a[p.unused_dofs])                                # exactly zero: the reciprocal of these is the caller's
