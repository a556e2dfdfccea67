"""Recovered quantities (fh_recover*, fenris_amd.recovery): displacement gradient, strain, stresses, energy
density and element volumes at points, elements and nodes -- against closed forms for affine fields, against the numpy restatement of
tests/recovery_reference.py for smooth fields, per-point and compact tables, element masks and high-valence nodes, and against the
engine's own energy, volume and physical points.

Tolerance: the project's parity tolerance TOL = 1e-12 (tests/test_gpu_parity.py), max|got - ref| <= TOL max|ref| per quantity, absolute
1e-13 where the reference vanishes: both sides evaluate the same formulas in double and differ in FMA use and summation order only.

Row pairing with fh_physical_quadrature_points: the gradient of the nodal interpolant of u = x (.) x is 2 x_q on the diagonal only where
the element's space holds x^2 -- Tet10 and Hex27 here.  A trilinear Hex8 does not hold it (the interpolant's gradient is off by O(h), not
by rounding), so the Hex8 case pairs the rows with a field its space does hold on the axis-aligned box mesh, u_k = x_(k+1) x_(k+2):
d u_k / d x_(k+1) = x_(k+2) at the point, to the same tolerance.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import recovery_reference as rr  # noqa: E402

TOL = 1e-12
ABS0 = 1e-13
LAME = (4.0e5, 6.0e5)
ALL_KINDS = list(rr.KINDS)
SOLID_OPS = ["LINEAR_ELASTIC", "NEO_HOOKEAN", "STVK"]
WHERE = ("points", "elements", "nodes")


def close(got, ref, what=""):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if ref.size == 0:
        return
    scale = np.abs(ref).max()
    err = np.abs(got - ref).max()
    print(f"{what}: max|got - ref| = {err:.3e}, max|ref| = {scale:.3e}")
    assert err <= (TOL * scale if scale > 0.0 else ABS0), (what, err, scale)


_CACHE = {}


def case(oracle, kind, op, field, perturb=0.1):
    """mesh, rule, u and the reference of one (kind, operator, field), computed once"""
    key = (kind, op, field, perturb)
    if key not in _CACHE:
        k, o = rr.KINDS[kind], rr.OPS[op]
        v, c = rr.mesh(oracle, k, perturb)
        w, p = rr.rule(oracle, k)
        d = v.shape[1]
        s = 1 if o == rr.LAPLACE else d
        if field == "affine":
            A, b = rr.affine_matrix(o, d)
            u = rr.affine_field(v, A, b)
        else:
            A, u = None, rr.smooth_field(v, s)
        _CACHE[key] = dict(v=v, c=c, w=w, p=p, u=u, A=A, ref=rr.recover(oracle, k, o, v, c, w, p, LAME, u))
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------------------- no GPU
@pytest.mark.parametrize("op", ["LAPLACE"] + SOLID_OPS)
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_reference_affine_closed_form(oracle, kind, op):
    """u = A x + b: every point, element and node value is the tensor of A (grad u = A^T), on meshes whose J varies per point"""
    cs = case(oracle, kind, op, "affine")
    o, A = rr.OPS[op], cs["A"]
    exact = rr.point_quantities(oracle, o, A.T.copy(), *LAME)
    if op == "LINEAR_ELASTIC":   # the closed form written out, independent of the oracle's materials
        mu, lam = LAME
        close(exact["cauchy_stress"], mu * (A + A.T) + lam * np.trace(A) * np.eye(len(A)), "sigma(A)")
        close(exact["energy_density"], mu * np.sum((0.5 * (A + A.T)) ** 2) + 0.5 * lam * np.trace(A) ** 2, "psi(A)")
    if op == "LAPLACE":
        close(exact["stress_pk1"], A, "flux(A)")
    for q in rr.quantities_of(o):
        for where in WHERE:
            ref = cs["ref"][q][where]
            close(ref, np.broadcast_to(np.asarray(exact[q]), ref.shape), f"{kind} {op} {q} {where}")
    vol = 1.0
    close(cs["ref"]["volume"].sum(), vol, "volume")


@pytest.mark.parametrize("kind,op", [("HEX8", "NEO_HOOKEAN"), ("TET10", "NEO_HOOKEAN"), ("QUAD9", "STVK"), ("TRI3", "LAPLACE")])
def test_reference_energy_is_the_assembled_scalar(oracle, kind, op):
    """sum_e V_e mean psi_e is the energy oracle.assemble_scalar integrates"""
    cs = case(oracle, kind, op, "smooth")
    asm = oracle.ElementAssembler(rr.KINDS[kind], rr.OPS[op], cs["v"], cs["c"], cs["w"], cs["p"],
                                  params=None if op == "LAPLACE" else LAME, u=cs["u"])
    st, _, energy = oracle.assemble_scalar(asm)
    assert st == 0
    ref = cs["ref"]
    close(np.sum(ref["volume"] * ref["energy_density"]["elements"]), energy, f"{kind} {op} energy")


def test_abi_names():
    import fenris_amd as fa
    from fenris_amd import _ffi

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "fenris_hip.h")).read()
    for name in ("fh_recover_components", "fh_recover_rows", "fh_recover_dev", "fh_recover"):
        assert name in _ffi.exported_symbols() and name + "(" in header
    assert hasattr(fa, "Recovery") and hasattr(fa.Engine, "recover")
    assert "#define FH_ABI_VERSION 1" in header


# ---------------------------------------------------------------------------------------------------------------- GPU
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    import fenris_amd as fa

    eng = fa.Engine(0)
    yield eng
    eng.close()


def _operator(op):
    import fenris_amd as fa

    return {"LAPLACE": lambda: fa.LaplaceOperator(), "LINEAR_ELASTIC": lambda: fa.MaterialEllipticOperator(fa.LinearElasticMaterial()),
            "NEO_HOOKEAN": lambda: fa.MaterialEllipticOperator(fa.NeoHookeanMaterial()),
            "STVK": lambda: fa.MaterialEllipticOperator(fa.StVKMaterial())}[op]()


def setup(engine, kind, op, v, c, w, p, u, table=None):
    """the context as the residual would see it; table: a quadrature table, or None for uniform LAME data"""
    import fenris_amd as fa

    mesh = fa.Mesh(v, c, rr.KINDS[kind])
    if table is None:
        table = fa.UniformQuadratureTable.from_points_and_weights(p, w)
        if op != "LAPLACE":
            table = table.with_uniform_data(fa.LameParameters(*LAME))
    return (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(mesh).with_operator(_operator(op))
            .with_quadrature_table(table).with_u(u).build())


def host(t):
    return t.cpu().numpy()


def check_all(engine, ref, op, what, where=WHERE):
    for q in rr.quantities_of(rr.OPS[op]):
        for loc in where:
            close(host(engine.recover(q, loc)), ref[q][loc], f"{what} {q} {loc}")
    close(host(engine.recover("volume", "elements")), ref["volume"], f"{what} volume")


@gpu
@pytest.mark.parametrize("op", ["LAPLACE"] + SOLID_OPS)
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_affine_field_is_the_closed_form(engine, oracle, kind, op):
    cs = case(oracle, kind, op, "affine")
    setup(engine, kind, op, cs["v"], cs["c"], cs["w"], cs["p"], cs["u"])
    exact = rr.point_quantities(oracle, rr.OPS[op], cs["A"].T.copy(), *LAME)
    for q in rr.quantities_of(rr.OPS[op]):
        for loc in WHERE:
            got = host(engine.recover(q, loc))
            close(got, np.broadcast_to(np.asarray(exact[q]), got.shape), f"{kind} {op} {q} {loc}")
    close(host(engine.recover("volume", "elements")), cs["ref"]["volume"], f"{kind} volume")


@gpu
@pytest.mark.parametrize("op", ["LAPLACE"] + SOLID_OPS)
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_smooth_field_matches_reference(engine, oracle, kind, op):
    cs = case(oracle, kind, op, "smooth")
    setup(engine, kind, op, cs["v"], cs["c"], cs["w"], cs["p"], cs["u"])
    check_all(engine, cs["ref"], op, f"{kind} {op}")


@gpu
@pytest.mark.parametrize("kind,op", [("HEX8", "NEO_HOOKEAN"), ("TET10", "STVK"), ("QUAD4", "LINEAR_ELASTIC"), ("HEX27", "LINEAR_ELASTIC")])
def test_per_point_and_compact_tables(engine, oracle, kind, op):
    import fenris_amd as fa

    cs = case(oracle, kind, op, "smooth")
    v, c, w, p, u = (cs[k] for k in "vcwpu")
    nq, E = len(w), len(c)
    # Lame parameters that differ per point ...
    per_point = np.stack([LAME[0] * (1.0 + 0.25 * np.arange(nq) / nq), LAME[1] * (1.0 - 0.3 * np.arange(nq) / nq)], axis=1)
    table = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_data([tuple(x) for x in per_point])
    setup(engine, kind, op, v, c, w, p, u, table)
    ref = rr.recover(oracle, rr.KINDS[kind], rr.OPS[op], v, c, w, p, per_point, u)
    check_all(engine, ref, op, f"{kind} {op} per-point")
    assert np.abs(ref["stress_pk1"]["points"] - cs["ref"]["stress_pk1"]["points"]).max() > 1e-3 * np.abs(ref["stress_pk1"]["points"]).max()
    # ... and per element and point: three rules of a compact table
    rules = np.stack([per_point * f for f in (1.0, 1.7, 0.6)])
    e2r = np.arange(E, dtype=np.uint64) % 3
    compact = fa.CompactQuadratureTable(p, w, [[tuple(x) for x in r] for r in rules], e2r)
    setup(engine, kind, op, v, c, w, p, u, compact)
    refc = rr.recover(oracle, rr.KINDS[kind], rr.OPS[op], v, c, w, p, (rules, e2r), u)
    check_all(engine, refc, op, f"{kind} {op} compact")
    # uniform data and a per-point table of the same constants are the same call into the library (the residual makes no difference
    # between them either: both arrive as one nq x 2 table): the same bits.  A compact table of one constant rule takes the rule-map
    # path: equal to TOL.
    setup(engine, kind, op, v, c, w, p, u)
    uni = {loc: host(engine.recover("stress_pk1", loc)) for loc in WHERE}
    filled = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_data([LAME] * nq)
    setup(engine, kind, op, v, c, w, p, u, filled)
    for loc in WHERE:
        assert np.array_equal(host(engine.recover("stress_pk1", loc)), uni[loc])
    one = fa.CompactQuadratureTable(p, w, [[LAME] * nq], np.zeros(E, dtype=np.uint64))
    setup(engine, kind, op, v, c, w, p, u, one)
    for loc in WHERE:
        close(host(engine.recover("stress_pk1", loc)), uni[loc], f"{kind} one-rule compact {loc}")


@gpu
@pytest.mark.parametrize("kind", ["HEX8", "TET10"])
def test_consistent_with_energy_volume_and_points(engine, oracle, kind):
    op = "NEO_HOOKEAN"
    cs = case(oracle, kind, op, "smooth")
    asm = setup(engine, kind, op, cs["v"], cs["c"], cs["w"], cs["p"], cs["u"])
    vol = host(engine.recover("volume", "elements"))
    psi = host(engine.recover("energy_density", "elements"))
    close(np.sum(vol * psi), asm.engine.assemble_scalar(), f"{kind} energy")
    close(vol.sum(), 1.0, f"{kind} volume")


@gpu
@pytest.mark.parametrize("kind", ["HEX8", "TET10", "HEX27"])
def test_point_rows_pair_with_physical_points(engine, oracle, kind):
    op = "NEO_HOOKEAN"
    k = rr.KINDS[kind]
    v, c = rr.mesh(oracle, k, perturb=0.0 if kind == "HEX8" else 0.1)
    w, p = rr.rule(oracle, k)
    if kind == "HEX8":   # a field of the trilinear space (module docstring)
        u = np.stack([v[:, 1] * v[:, 2], v[:, 2] * v[:, 0], v[:, 0] * v[:, 1]], axis=1).reshape(-1)
    else:
        u = (v * v).reshape(-1)
    setup(engine, kind, op, v, c, w, p, u)
    x = np.asarray(engine.physical_quadrature_points(len(w))).reshape(-1, 3)
    g = host(engine.recover("grad_u", "points"))
    assert g.shape == (len(c) * len(w), 3, 3)
    if kind == "HEX8":
        got = np.stack([g[:, (i + 1) % 3, i] for i in range(3)], axis=1)    # d u_i / d x_(i+1) = x_(i+2)
        close(got, np.stack([x[:, (i + 2) % 3] for i in range(3)], axis=1), f"{kind} pairing")
    else:
        close(np.stack([g[:, i, i] for i in range(3)], axis=1), 2.0 * x, f"{kind} pairing")


@gpu
@pytest.mark.parametrize("kind,op", [("HEX8", "LINEAR_ELASTIC"), ("TET10", "NEO_HOOKEAN"), ("TRI3", "STVK"), ("QUAD9", "LAPLACE")])
def test_element_mask(engine, oracle, kind, op):
    cs = case(oracle, kind, op, "smooth")
    setup(engine, kind, op, cs["v"], cs["c"], cs["w"], cs["p"], cs["u"])
    E, nq = len(cs["c"]), len(cs["w"])
    mask = (np.arange(E) % 2 == 0).astype(np.uint8)
    if kind == "TRI3":   # orphan some nodes: the whole first row of cells is masked too
        mask[: 6] = 0
    engine.set_active_elements(mask)
    try:
        ref = rr.recover(oracle, rr.KINDS[kind], rr.OPS[op], cs["v"], cs["c"], cs["w"], cs["p"], LAME, cs["u"], mask=mask)
        check_all(engine, ref, op, f"{kind} {op} masked")
        g = host(engine.recover("grad_u", "points")).reshape(E, nq, -1)
        assert np.all(g[mask == 0] == 0.0) and np.all(host(engine.recover("volume", "elements"))[mask == 0] == 0.0)
        touched = np.zeros(len(cs["v"]), dtype=bool)
        touched[np.unique(cs["c"][mask == 1])] = True
        if kind == "TRI3":
            assert not touched.all()
        assert np.all(host(engine.recover("grad_u", "nodes"))[~touched] == 0.0)
    finally:
        engine.set_active_elements(None)


@gpu
@pytest.mark.parametrize("shape", ["quad", "tet"])
def test_high_valence_hub(engine, oracle, shape):
    """the fans of tests/test_high_valence.py: 64 elements around one node"""
    from test_high_valence import quad_fan, tet_fan

    m = quad_fan(64) if shape == "quad" else tet_fan(64)
    kind = "QUAD4" if shape == "quad" else "TET4"
    v, c = m.vertices, m.connectivity
    w, p = rr.rule(oracle, rr.KINDS[kind])
    u = rr.smooth_field(v, v.shape[1])
    setup(engine, kind, "NEO_HOOKEAN", v, c, w, p, u)
    ref = rr.recover(oracle, rr.KINDS[kind], rr.NEO_HOOKEAN, v, c, w, p, LAME, u)
    assert np.sum(c == 0) == 64
    for q in ("cauchy_stress", "von_mises", "grad_u"):
        got = host(engine.recover(q, "nodes"))
        close(got[0], ref[q]["nodes"][0], f"{shape} fan hub {q}")
        close(got, ref[q]["nodes"], f"{shape} fan {q}")


@gpu
def test_inverted_element(engine, oracle):
    """one Tet4 with det F < 0 under NeoHookean: NaN in P and sigma, +inf in psi, there and nowhere else, and no error code"""
    v, c = rr.mesh(oracle, rr.TET4)
    w, p = rr.rule(oracle, rr.TET4)
    ci = c.astype(np.int64)

    def det_f(u):   # F of every (affine) tetrahedron from its deformed edges
        return np.array([np.linalg.det((((v + u)[e[1:]] - (v + u)[e[0]]).T) @ np.linalg.inv((v[e[1:]] - v[e[0]]).T)) for e in ci])

    # a vertex pushed 5 % past its opposite face inverts that element; its neighbours share the vertex and flatten, so take the first
    # (element, vertex) that inverts exactly one element and leaves det F >= 0.01 in every other
    u, e0 = None, -1
    for e in range(len(ci)):
        for la in range(4):
            cand = np.zeros_like(v)
            cand[ci[e, la]] = 1.05 * (v[np.delete(ci[e], la)].mean(axis=0) - v[ci[e, la]])
            dets = det_f(cand)
            if u is None and dets[e] < 0.0 and np.sum(dets <= 0.0) == 1 and np.delete(dets, e).min() >= 0.01:
                u, e0 = cand, e
    assert u is not None
    setup(engine, "TET4", "NEO_HOOKEAN", v, c, w, p, u.reshape(-1))
    ref = rr.recover(oracle, rr.TET4, rr.NEO_HOOKEAN, v, c, w, p, LAME, u.reshape(-1))
    bad = np.isnan(ref["stress_pk1"]["elements"]).any(axis=(1, 2))
    assert bad[e0] and bad.sum() == 1
    P = host(engine.recover("stress_pk1", "elements"))
    sg = host(engine.recover("cauchy_stress", "elements"))
    psi = host(engine.recover("energy_density", "elements"))
    for e in range(len(c)):
        if bad[e]:
            assert np.isnan(P[e]).all() and np.isnan(sg[e]).all() and psi[e] == np.inf
        else:
            assert np.isfinite(P[e]).all() and np.isfinite(sg[e]).all() and np.isfinite(psi[e])
    close(P[~bad], ref["stress_pk1"]["elements"][~bad], "finite elements")
    assert np.isfinite(host(engine.recover("grad_u", "elements"))).all()


@gpu
def test_determinism_and_small_meshes(engine, oracle):
    import fenris_amd as fa

    cs = case(oracle, "HEX27", "STVK", "smooth")
    setup(engine, "HEX27", "STVK", cs["v"], cs["c"], cs["w"], cs["p"], cs["u"])
    for q in ("cauchy_stress", "von_mises"):
        assert np.array_equal(host(engine.recover(q, "nodes")), host(engine.recover(q, "nodes")))
    # the host entry point gives what the device one gives
    out = np.zeros((len(cs["v"]), 3, 3))
    engine._check(engine._lib.fh_recover(engine._h, fa._ffi.RECOVER_STRAIN, fa._ffi.AT_NODES, fa._ffi.fp(out)))
    assert np.array_equal(out, host(engine.recover("strain", "nodes")))
    assert isinstance(fa.Recovery(engine).element_volumes().shape, tuple) and fa.Recovery(engine).von_mises("points").is_cuda
    # no u: zero strain and zero stress
    setup(engine, "HEX27", "STVK", cs["v"], cs["c"], cs["w"], cs["p"], None)
    for q in ("strain", "stress_pk1", "cauchy_stress", "von_mises", "energy_density"):
        for loc in WHERE:
            assert np.all(host(engine.recover(q, loc)) == 0.0)
    # one element, and none
    for kind in ("TET4", "QUAD9"):
        v, c = rr.mesh(oracle, rr.KINDS[kind])
        w, p = rr.rule(oracle, rr.KINDS[kind])
        u = rr.smooth_field(v, v.shape[1])
        setup(engine, kind, "LINEAR_ELASTIC", v, c[:1], w, p, u)
        ref = rr.recover(oracle, rr.KINDS[kind], rr.LINEAR_ELASTIC, v, c[:1], w, p, LAME, u)
        check_all(engine, ref, "LINEAR_ELASTIC", f"one {kind}")
        setup(engine, kind, "LINEAR_ELASTIC", v, c[:0], w, p, u)
        assert engine.recover("strain", "points").shape == (0, v.shape[1], v.shape[1])
        assert engine.recover("volume", "elements").shape == (0,)
        assert np.all(host(engine.recover("strain", "nodes")) == 0.0)


@gpu
def test_error_codes(engine, oracle):
    import ctypes as C

    import fenris_amd as fa
    from fenris_amd import _ffi

    lib = engine._lib
    nc = C.c_uint32(0)
    fresh = fa.Engine(0)
    try:   # nothing set
        assert lib.fh_recover_components(fresh._h, _ffi.RECOVER_STRAIN, C.byref(nc)) == _ffi.FH_INVALID_STATE
        buf = np.zeros(16)
        assert lib.fh_recover(fresh._h, _ffi.RECOVER_STRAIN, _ffi.AT_POINTS, _ffi.fp(buf)) == _ffi.FH_INVALID_STATE
        v, c = rr.mesh(oracle, rr.QUAD4)
        fresh.set_mesh(fa.Mesh(v, c, fa.QUAD4))
        assert lib.fh_recover(fresh._h, _ffi.RECOVER_STRAIN, _ffi.AT_POINTS, _ffi.fp(buf)) == _ffi.FH_INVALID_STATE   # no operator
        fresh.set_operator(_ffi.LINEAR_ELASTIC)
        assert lib.fh_recover(fresh._h, _ffi.RECOVER_STRAIN, _ffi.AT_POINTS, _ffi.fp(buf)) == _ffi.FH_INVALID_STATE   # no table
    finally:
        fresh.close()
    cs = case(oracle, "QUAD4", "LINEAR_ELASTIC", "smooth")
    v, c, w, p, u = (cs[k] for k in "vcwpu")
    setup(engine, "QUAD4", "LINEAR_ELASTIC", v, c, w, p, u)
    assert lib.fh_recover_components(engine._h, _ffi.RECOVER_GRAD_U, C.byref(nc)) == _ffi.FH_OK and nc.value == 4
    assert lib.fh_recover_components(engine._h, _ffi.RECOVER_VON_MISES, C.byref(nc)) == _ffi.FH_OK and nc.value == 1
    big = np.zeros(len(c) * len(w) * 4)
    for q, where in ((7, _ffi.AT_POINTS), (-1, _ffi.AT_POINTS), (_ffi.RECOVER_STRAIN, 3), (_ffi.RECOVER_STRAIN, -1),
                     (_ffi.RECOVER_VOLUME, _ffi.AT_POINTS), (_ffi.RECOVER_VOLUME, _ffi.AT_NODES)):
        assert lib.fh_recover(engine._h, q, where, _ffi.fp(big)) == _ffi.FH_BAD_ARGUMENT, (q, where)
    assert lib.fh_recover(engine._h, _ffi.RECOVER_STRAIN, _ffi.AT_POINTS, None) == _ffi.FH_BAD_ARGUMENT
    with pytest.raises(ValueError):
        engine.recover("stress", "points")
    with pytest.raises(fa.FenrisError) as bad:
        engine.recover("volume", "nodes")
    assert bad.value.code == _ffi.FH_BAD_ARGUMENT
    # Laplace has no strain, Cauchy or von Mises stress
    setup(engine, "QUAD4", "LAPLACE", v, c, w, p, u[: len(v)])
    for q in (_ffi.RECOVER_STRAIN, _ffi.RECOVER_STRESS_CAUCHY, _ffi.RECOVER_VON_MISES):
        assert lib.fh_recover_components(engine._h, q, C.byref(nc)) == _ffi.FH_UNSUPPORTED
        assert lib.fh_recover(engine._h, q, _ffi.AT_ELEMENTS, _ffi.fp(big)) == _ffi.FH_UNSUPPORTED
    assert lib.fh_recover_components(engine._h, _ffi.RECOVER_STRESS_PK1, C.byref(nc)) == _ffi.FH_OK and nc.value == 2
    # the mass operators and FH_TENSOR
    for opk in (_ffi.MASS_SCALAR, _ffi.MASS_VECTOR, _ffi.TENSOR):
        engine.set_operator(opk)
        assert lib.fh_recover_components(engine._h, _ffi.RECOVER_GRAD_U, C.byref(nc)) == _ffi.FH_UNSUPPORTED
        assert lib.fh_recover(engine._h, _ffi.RECOVER_GRAD_U, _ffi.AT_ELEMENTS, _ffi.fp(big)) == _ffi.FH_UNSUPPORTED
    # a rule-set table, at every location, with the wording of fh_physical_quadrature_points
    setup(engine, "QUAD4", "LINEAR_ELASTIC", v, c, w, p, u)
    w1, p1 = oracle.quadrilateral_gauss(1)
    lame = fa.LameParameters(*LAME)
    table = fa.GeneralQuadratureTable.from_points_weights_and_data([p if e % 2 else p1 for e in range(len(c))],
                                                                   [w if e % 2 else w1 for e in range(len(c))],
                                                                   [[lame] * (len(w) if e % 2 else 1) for e in range(len(c))])
    engine.set_quadrature_table(table)
    for where in (_ffi.AT_POINTS, _ffi.AT_ELEMENTS, _ffi.AT_NODES):
        assert lib.fh_recover(engine._h, _ffi.RECOVER_STRAIN, where, _ffi.fp(big)) == _ffi.FH_UNSUPPORTED
        assert "rule-set quadrature tables (fh_set_quadrature_rules) are not walked here" in engine.last_error()
    # a singular Jacobian in an active element, reported as the residual reports it
    vs = v.copy()
    vs[c[2]] = 0.5   # (a power of two: every product of J = X G^T is exact, so det J is 0 exactly)
    setup(engine, "QUAD4", "LINEAR_ELASTIC", vs, c, w, p, u)
    with pytest.raises(fa.SingularJacobianError):
        engine.recover("strain", "elements")
    with pytest.raises(fa.SingularJacobianError):
        engine.recover("strain", "points")
