"""Degree elevation on the device (fh_elevate_degree, Engine.elevate_degree, elevate_degree_with_transfer): Tet4 -> Tet10, Tri3 -> Tri6,
Quad4 -> Quad9, Hex8 -> Hex20 and Hex8 -> Hex27.  Mesh and vertices bit-identical to the host converters (fh_refine_to_quadratic,
fh_hex8_to_hex27), the transfer against a NumPy construction from the parent tables of include/fenris_hip.h, the round trip through
fh_coarsen_degree, the device-to-device path, a multigrid solve on a hierarchy that starts from the linear meshes, and the status codes."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import fenris_amd as fa
from fenris_amd import _ffi, quadrature

FH_BAD_ARGUMENT, FH_INVALID_STATE, FH_UNSUPPORTED = 2, 5, 6
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("fh_elevate_degree", "fh_degree_elevation_mesh", "fh_degree_elevation_transfer", "fh_set_mesh_from_degree_elevation")
EPS = np.finfo(np.float64).eps

_HEX_EDGES = ((0, 1), (0, 3), (0, 4), (1, 2), (1, 5), (2, 3), (2, 6), (3, 7), (4, 5), (4, 7), (5, 6), (6, 7))
_HEX_FACES = ((0, 1, 2, 3), (0, 1, 4, 5), (0, 3, 4, 7), (1, 2, 5, 6), (2, 3, 6, 7), (4, 5, 6, 7))
# high kind -> (linear kind, vertex slots, parents of the other local nodes as local nodes): the coarsening section of the header
TABLES = {
    fa.TET10: (fa.TET4, 4, ((0, 1), (1, 2), (0, 2), (0, 3), (2, 3), (1, 3))),
    fa.TRI6: (fa.TRI3, 3, ((0, 1), (1, 2), (0, 2))),
    fa.QUAD9: (fa.QUAD4, 4, ((0, 1), (1, 2), (2, 3), (0, 3), (0, 1, 2, 3))),
    fa.HEX20: (fa.HEX8, 8, _HEX_EDGES),
    fa.HEX27: (fa.HEX8, 8, _HEX_EDGES + _HEX_FACES + (tuple(range(8)),)),
}
HOST = {fa.TET10: fa.tet10_mesh_from_tet4, fa.TRI6: fa.tri6_mesh_from_tri3, fa.QUAD9: fa.quad9_mesh_from_quad4,
        fa.HEX20: fa.hex20_mesh_from_hex8, fa.HEX27: fa.hex27_mesh_from_hex8}
TO_KINDS = {fa.TET4: (fa.TET10,), fa.TRI3: (fa.TRI6,), fa.QUAD4: (fa.QUAD9,), fa.HEX8: (fa.HEX20, fa.HEX27)}
KIND_NAME = {fa.TET10: "tet10", fa.TRI6: "tri6", fa.QUAD9: "quad9", fa.HEX20: "hex20", fa.HEX27: "hex27"}
KEEPS_VERTICES = (fa.TRI6, fa.QUAD9)


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
def perturbed(mesh, amp, seed):
    rng = np.random.default_rng(seed)
    return fa.Mesh(mesh.vertices + amp * rng.uniform(-1.0, 1.0, mesh.vertices.shape), mesh.connectivity, mesh.elem_kind)


def permuted(mesh, seed):
    """the vertex numbers and the cell order permuted: first-occurrence order, key order and index order all differ"""
    rng = np.random.default_rng(seed)
    perm = rng.permutation(mesh.num_nodes())           # new -> old
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    cells = rng.permutation(mesh.num_elements())
    return fa.Mesh(mesh.vertices[perm], inv[mesh.connectivity.astype(np.int64)][cells].astype(np.uint64), mesh.elem_kind)


def with_unused_vertex(mesh):
    """one more vertex, of no cell, in the middle of the numbering"""
    at = mesh.num_nodes() // 2
    v = np.insert(mesh.vertices, at, np.full(mesh.vertices.shape[1], 7.25), axis=0)
    c = mesh.connectivity.astype(np.int64)
    return fa.Mesh(v, (c + (c >= at)).astype(np.uint64), mesh.elem_kind)


def _quad_3x2():
    return perturbed(fa.procedural.create_rectangular_uniform_quad_mesh_2d(1.0, 3, 2, 1, np.array([0.0, 2.0])), 0.05, 5)


def _tri_3x2():
    q = _quad_3x2()
    c = q.connectivity
    tri = np.stack([c[:, [0, 1, 2]], c[:, [0, 2, 3]]], axis=1).reshape(-1, 3)
    return fa.Mesh(q.vertices, np.ascontiguousarray(tri, dtype=np.uint64), fa.TRI3)


def _one(kind, v):
    v = np.asarray(v, dtype=np.float64)
    return perturbed(fa.Mesh(v, np.arange(len(v), dtype=np.uint64).reshape(1, -1), kind), 0.1, len(v))


BASE = {
    "one_tet4": lambda: _one(fa.TET4, [[-1, -1, -1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]),
    "one_tri3": lambda: _one(fa.TRI3, [[-1, -1], [1, -1], [-1, 1]]),
    "one_quad4": lambda: _one(fa.QUAD4, [[-1, -1], [1, -1], [1, 1], [-1, 1]]),
    "one_hex8": lambda: _one(fa.HEX8, [[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]]),
    "hex8_2x2x2": lambda: perturbed(fa.procedural.create_unit_box_uniform_hex_mesh_3d(2), 0.05, 3),
    "hex8_3x2x1": lambda: perturbed(fa.procedural.create_rectangular_uniform_hex_mesh(1.0, 3, 2, 1, 1), 0.1, 4),
    "tet4_bcc1": lambda: fa.procedural.create_unit_box_uniform_tet_mesh_3d(1),
    "tet4_bcc2": lambda: perturbed(fa.procedural.create_unit_box_uniform_tet_mesh_3d(2), 0.02, 6),
    "tet4_sphere593": lambda: fa.io.load_msh_from_file(os.path.join(GOLDEN, "msh", "sphere_tet4_593.msh"), fa.TET4),
    "quad4_3x2": _quad_3x2,
    "tri3_3x2": _tri_3x2,
}
MESHES = {
    **BASE,
    **{name + "_permuted": (lambda f=f, k=k: permuted(f(), 51 + k)) for k, (name, f) in enumerate(sorted(BASE.items()))},
    **{name + "_unused": (lambda name=name: with_unused_vertex(permuted(BASE[name](), 71)))
       for name in ("tet4_bcc1", "hex8_3x2x1", "quad4_3x2", "tri3_3x2")},
}
_KIND_OF = {"tet4": fa.TET4, "tri3": fa.TRI3, "quad4": fa.QUAD4, "hex8": fa.HEX8}


def _linear_kind(name):
    return next(k for key, k in _KIND_OF.items() if key in name)


CASES = [(name, to) for name in sorted(MESHES) for to in TO_KINDS[_linear_kind(name)]]
CASE_IDS = [f"{name}-{KIND_NAME[to]}" for name, to in CASES]
WITHOUT_UNUSED = [(c, i) for c, i in zip(CASES, CASE_IDS) if not (c[0].endswith("_unused") and c[1] in KEEPS_VERTICES)]


@pytest.fixture(scope="module")
def engine():
    eng = fa.Engine(0)
    yield eng
    eng.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def table_transfer(lin, high):
    """the transfer from the parent tables, sequentially: (offsets, indices, weights) by node of `high` over the vertices of `lin`"""
    _, nv, parents = TABLES[high.elem_kind]
    slots = tuple((a,) for a in range(nv)) + parents
    rows = {}
    lc, hc = lin.connectivity.astype(np.int64).tolist(), high.connectivity.astype(np.int64).tolist()
    for cl, ch in zip(lc, hc):
        for l, par in enumerate(slots):
            rows.setdefault(ch[l], tuple(sorted(cl[a] for a in par)))
    if high.elem_kind in KEEPS_VERTICES:
        for i in range(lin.num_nodes()):
            rows.setdefault(i, (i,))
    off, idx, w = [0], [], []
    for i in range(high.num_nodes()):
        idx += rows[i]
        w += [1.0 / len(rows[i])] * len(rows[i])
        off.append(len(idx))
    return np.array(off, dtype=np.uint64), np.array(idx, dtype=np.uint64), np.array(w, dtype=np.float64)


# ---- 1. bit identity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,to_kind", CASES, ids=CASE_IDS)
def test_bit_identical_to_the_host_converters(engine, name, to_kind):
    lin = MESHES[name]()
    ref = HOST[to_kind](lin)
    high, t = fa.elevate_degree_with_transfer(lin, to_kind, engine)
    assert high.elem_kind == to_kind and high.num_nodes() == ref.num_nodes() and high.num_elements() == lin.num_elements()
    assert np.array_equal(high.connectivity, ref.connectivity)
    assert np.array_equal(bits(high.vertices), bits(ref.vertices))
    if name.endswith("_unused"):
        kept = to_kind in KEEPS_VERTICES
        used = len(np.unique(lin.connectivity))
        assert used == lin.num_nodes() - 1
        assert len(np.where(np.diff(t.offsets.astype(np.int64)) == 1)[0]) == (lin.num_nodes() if kept else used)
        assert (np.all(high.vertices == 7.25, axis=1)).any() == kept
    sizes = engine.elevate_degree(to_kind)                  # the same mesh again: the same bits
    high2, t2 = engine.degree_elevation()
    assert sizes == (high.num_nodes(), len(t.indices))
    assert np.array_equal(high2.connectivity, high.connectivity) and np.array_equal(bits(high2.vertices), bits(high.vertices))
    assert np.array_equal(t2.offsets, t.offsets) and np.array_equal(t2.indices, t.indices) and np.array_equal(bits(t2.weights), bits(t.weights))


@pytest.mark.gpu
def test_the_sphere_spans_several_workgroups(engine):
    lin = MESHES["tet4_sphere593"]()
    assert lin.num_elements() == 593 and (10 * 593) % 256 != 0 and 10 * 593 > 256
    high = fa.elevate_degree(lin, fa.TET10, engine)
    assert high.num_elements() == 593 and high.num_nodes() > lin.num_nodes()


@pytest.mark.gpu
def test_default_engine():
    lin = MESHES["quad4_3x2_permuted"]()
    ref = fa.quad9_mesh_from_quad4(lin)
    high, t = fa.elevate_degree_with_transfer(lin, fa.QUAD9)
    assert np.array_equal(high.connectivity, ref.connectivity) and np.array_equal(bits(high.vertices), bits(ref.vertices))
    assert fa.elevate_degree(lin, fa.QUAD9).num_nodes() == ref.num_nodes() and t.num_coarse == lin.num_nodes()


# ---- 2. the transfer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,to_kind", CASES, ids=CASE_IDS)
def test_transfer(engine, name, to_kind):
    lin = MESHES[name]()
    high, t = fa.elevate_degree_with_transfer(lin, to_kind, engine)
    off, idx, w = table_transfer(lin, high)
    assert t.num_coarse == lin.num_nodes() and t.num_fine == high.num_nodes()
    assert np.array_equal(t.offsets, off) and np.array_equal(t.indices, idx) and np.array_equal(bits(t.weights), bits(w))
    o = t.offsets.astype(np.int64)
    counts = np.diff(o)
    assert set(counts.tolist()) <= {1, 2, 4, 8}
    assert np.array_equal(bits(t.weights), bits(np.repeat(1.0 / counts, counts)))            # exactly 1 / count
    inner = np.ones(len(t.indices), dtype=bool)
    inner[o[:-1]] = False
    assert (np.diff(t.indices.astype(np.int64))[inner[1:]] > 0).all()                       # parents strictly ascending within a row
    # the positions and an affine function of them, through P.  The coefficients are powers of two: their products with the
    # coordinates are exact, so the function's own rounding stays within the bound that the positions have
    scale = np.abs(high.vertices).max()
    assert np.abs(t.apply(lin.vertices) - high.vertices).max() <= 4 * EPS * scale
    a = np.array([0.25, -0.5, 0.125])[: lin.vertices.shape[1]]
    f_lin, f_high = lin.vertices @ a + 0.125, high.vertices @ a + 0.125
    assert np.abs(t.apply(f_lin) - f_high).max() <= 4 * EPS * scale


# ---- 3. round trip with the coarsener ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,to_kind", [c for c, _ in WITHOUT_UNUSED], ids=[i for _, i in WITHOUT_UNUSED])
def test_round_trip_with_the_coarsener(engine, name, to_kind):
    lin = MESHES[name]()
    high, t = fa.elevate_degree_with_transfer(lin, to_kind, engine)
    other = fa.Engine(0)
    try:
        lin2, t2, vn = fa.coarsen_degree_with_transfer(high, other)
    finally:
        other.close()
    # coarse vertex j is high node vn[j], whose elevation row names the linear vertex it came from
    o = t.offsets.astype(np.int64)
    vn = vn.astype(np.int64)
    assert (np.diff(o)[vn] == 1).all() and (t.weights[o[vn]] == 1.0).all()
    orig = t.indices[o[vn]].astype(np.int64)
    assert lin2.elem_kind == lin.elem_kind and len(np.unique(orig)) == len(orig) == lin2.num_nodes()
    assert np.array_equal(orig[lin2.connectivity.astype(np.int64)], lin.connectivity.astype(np.int64))
    assert np.array_equal(vn[lin2.connectivity.astype(np.int64)], high.connectivity[:, : lin.connectivity.shape[1]].astype(np.int64))
    assert np.array_equal(bits(lin2.vertices), bits(lin.vertices[orig]))
    # the two transfers, columns renamed by that map
    assert np.array_equal(t2.offsets, t.offsets)
    P, P2 = t.to_scipy().tocsc()[:, orig].tocsr(), t2.to_scipy()
    assert P.shape == P2.shape and (P != P2).nnz == 0
    if to_kind in KEEPS_VERTICES:
        assert np.array_equal(vn, np.arange(lin.num_nodes())) and np.array_equal(orig, vn)
        assert np.array_equal(t2.indices, t.indices)


# ---- 4. device to device -----------------------------------------------------------------------------------------------------------
def _matrix(eng, kind):
    """pattern and values in a fixed order of summation: Hex27 Laplace, Tet10 linear elasticity"""
    if kind == fa.HEX27:
        w, p = quadrature.tensor.hexahedron_gauss(3)
        eng.set_operator(_ffi.LAPLACE)
        eng.set_quadrature_uniform(np.asarray(w, dtype=np.float64), np.asarray(p, dtype=np.float64))
    else:
        w, p = quadrature.total_order.tetrahedron(2)
        lame = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.3))
        eng.set_operator(_ffi.LINEAR_ELASTIC)
        eng.set_quadrature_uniform(np.asarray(w, dtype=np.float64), np.asarray(p, dtype=np.float64),
                                   np.tile(np.asarray(lame.as_pair(), dtype=np.float64), (len(w), 1)))
    ro, ci = eng.pattern()
    vals = np.zeros(len(ci))
    eng.assemble_matrix(vals, fa.SCATTER_GATHER | fa.ASSEMBLE_REPRODUCIBLE)
    return ro, ci, vals


@pytest.mark.gpu
@pytest.mark.parametrize("name,to_kind", [("hex8_2x2x2", fa.HEX27), ("tet4_bcc2_permuted", fa.TET10)], ids=["hex27_laplace", "tet10_elastic"])
def test_set_mesh_from_degree_elevation_matches_host_arrays(engine, name, to_kind):
    lin = MESHES[name]()
    ref = HOST[to_kind](lin)
    high, _ = fa.elevate_degree_with_transfer(lin, to_kind, engine)       # the engine now holds the elevation
    a, b = fa.Engine(0), fa.Engine(0)
    try:
        a.set_mesh_from_degree_elevation(engine)
        assert a.num_nodes() == ref.num_nodes() and a.num_elements() == ref.num_elements()
        b.set_mesh(ref)
        (roa, cia, va), (rob, cib, vb) = _matrix(a, to_kind), _matrix(b, to_kind)
        assert np.array_equal(roa, rob) and np.array_equal(cia, cib)
        assert np.abs(vb).max() > 0.0 and np.abs(va - vb).max() <= 1e-12 * np.abs(vb).max()
        # the elevation is still held, and the engine can take it itself: it then holds none
        again, _ = engine.degree_elevation()
        assert np.array_equal(again.connectivity, high.connectivity)
        engine.set_mesh_from_degree_elevation(engine)
        assert engine.num_nodes() == ref.num_nodes() and engine.num_elements() == ref.num_elements()
        assert _ffi.lib().fh_degree_elevation_mesh(engine._h, None, None) == FH_INVALID_STATE
        assert _ffi.lib().fh_degree_elevation_transfer(engine._h, None, None, None) == FH_INVALID_STATE
    finally:
        a.close()
        b.close()


# ---- 5. multigrid ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_mg_pcg_on_a_hierarchy_from_the_linear_meshes():
    """Hex8 2^3 -> 4^3 by the device refiner, 4^3 -> Hex27 by the device elevation, whose transfer is the finest step as it is.  Laplace,
    u = 0 on the boundary.  Both solves stop at a relative residual of 1e-10; with a condition number of the order of 10^2 on this mesh
    their solutions agree to well within 1e-7 max |x|, the bound of the other MG-PCG tests."""
    eng, fine = fa.Engine(0), fa.Engine(0)
    try:
        linear, ts = fa.refine_uniformly_repeat_with_transfers(fa.procedural.create_unit_box_uniform_hex_mesh_3d(2), 1, eng)
        high, coarse, transfers = fa.degree_hierarchy_from_linear(linear, ts, fa.HEX27, eng)
        assert [m.num_elements() for m in coarse] == [8, 64] and high.num_elements() == 64 and high.num_nodes() == 729
        assert transfers[-1].num_coarse == coarse[-1].num_nodes() == 125 and transfers[-1].num_fine == 729
        assert coarse[-1] is linear[-1]                                       # no renumbering of the linear level
        ref = fa.hex27_mesh_from_hex8(linear[-1])
        assert np.array_equal(high.connectivity, ref.connectivity) and np.array_equal(bits(high.vertices), bits(ref.vertices))
        w, p = quadrature.tensor.hexahedron_gauss(3)
        qt = fa.UniformQuadratureTable.from_points_and_weights(p, w)
        asm = (fa.ElementEllipticAssemblerBuilder(fine).with_finite_element_space(high).with_operator(fa.LaplaceOperator())
               .with_quadrature_table(qt).with_u(np.zeros(high.num_nodes())).build())
        on_boundary = (np.isclose(high.vertices, 0.0) | np.isclose(high.vertices, 1.0)).any(axis=1)
        nodes = np.where(on_boundary)[0].astype(np.uint64)
        assert len(nodes) == 729 - 343
        b = np.ones(high.num_nodes())
        b[on_boundary] = 0.0
        mg = fa.GeometricMultigrid(asm, coarse, transfers)
        op = fa.MatrixFreeOperator(asm).with_dirichlet_nodes(nodes).with_multigrid(mg)
        x_mg, x_j = np.zeros_like(b), np.zeros_like(b)
        it_mg = op.cg_solve(b, x_mg, rel_tol=1e-10)
        it_j = op.cg_solve(b, x_j, fa.PRECOND_JACOBI, rel_tol=1e-10)
        print(f"hex27 laplace on 4^3 over Hex8 4^3 and 2^3: MG-PCG iterations {it_mg}, Jacobi-PCG iterations {it_j}")
        assert np.abs(x_j).max() > 0.0 and np.abs(x_mg - x_j).max() <= 1e-7 * np.abs(x_j).max()
        assert it_mg < it_j
        del mg
    finally:
        fine.close()
        eng.close()


# ---- 6. status codes ---------------------------------------------------------------------------------------------------------------
def _code(fn, *args):
    with pytest.raises(fa.FenrisError) as e:
        fn(*args)
    return e.value.code


def _nothing_held(eng):
    lib = _ffi.lib()
    assert lib.fh_degree_elevation_mesh(eng._h, None, None) == FH_INVALID_STATE
    assert lib.fh_degree_elevation_transfer(eng._h, None, None, None) == FH_INVALID_STATE
    assert _code(eng.degree_elevation) == FH_INVALID_STATE


@pytest.mark.gpu
def test_wrong_pairs_and_unsupported_kinds(engine):
    tet4, hex8, quad4, tri3 = (MESHES[k]() for k in ("tet4_bcc1", "one_hex8", "one_quad4", "one_tri3"))
    for mesh, to_kind in ((tet4, fa.HEX27), (tet4, fa.TET20), (tet4, fa.TET4), (tet4, 99), (tet4, -1), (hex8, fa.TET10), (hex8, fa.HEX8),
                          (quad4, fa.TRI6), (tri3, fa.QUAD9)):
        assert _code(fa.elevate_degree_with_transfer, mesh, to_kind, engine) == FH_BAD_ARGUMENT
        assert _code(fa.elevate_degree_with_transfer, mesh, to_kind) == FH_BAD_ARGUMENT
        _nothing_held(engine)
    for mesh in (fa.tet10_mesh_from_tet4(tet4), fa.tet20_mesh_from_tet4(tet4), fa.hex27_mesh_from_hex8(hex8), fa.quad9_mesh_from_quad4(quad4)):
        for to_kind in (fa.TET10, fa.HEX27, mesh.elem_kind):
            assert _code(fa.elevate_degree_with_transfer, mesh, to_kind, engine) == FH_UNSUPPORTED
            assert _code(fa.elevate_degree_with_transfer, mesh, to_kind) == FH_UNSUPPORTED
        _nothing_held(engine)
    engine.set_connectivity_ragged(1, 5, np.array([0, 3, 5], dtype=np.uint64), np.array([0, 1, 2, 3, 4], dtype=np.uint64))
    assert _code(engine.elevate_degree, fa.TET10) == FH_UNSUPPORTED
    _nothing_held(engine)
    high = fa.elevate_degree(tet4, fa.TET10, engine)          # the context stays usable
    assert np.array_equal(high.connectivity, fa.tet10_mesh_from_tet4(tet4).connectivity)


@pytest.mark.gpu
def test_lifetime_of_the_held_result():
    lib = _ffi.lib()
    eng, other = fa.Engine(0), fa.Engine(0)
    try:
        _nothing_held(eng)
        assert _code(other.set_mesh_from_degree_elevation, eng) == FH_INVALID_STATE
        lin = MESHES["hex8_3x2x1"]()
        eng.set_mesh(lin)
        _nothing_held(eng)
        eng.elevate_degree(fa.HEX27)
        high, t = eng.degree_elevation()
        # fh_update_vertices keeps it, with the positions it was formed from
        eng.update_vertices(lin.vertices * 3.0 + 1.0)
        kept, t_kept = eng.degree_elevation()
        assert np.array_equal(bits(kept.vertices), bits(high.vertices)) and np.array_equal(kept.connectivity, high.connectivity)
        assert np.array_equal(t_kept.indices, t.indices)
        # the next elevation replaces it
        eng.elevate_degree(fa.HEX20)
        assert eng.degree_elevation()[0].elem_kind == fa.HEX20
        moved = fa.hex20_mesh_from_hex8(fa.Mesh(lin.vertices * 3.0 + 1.0, lin.connectivity, fa.HEX8))
        assert np.array_equal(bits(eng.degree_elevation()[0].vertices), bits(moved.vertices))
        # fh_set_mesh drops it; so does fh_set_connectivity_ragged
        eng.set_mesh(lin)
        _nothing_held(eng)
        assert _code(other.set_mesh_from_degree_elevation, eng) == FH_INVALID_STATE
        eng.elevate_degree(fa.HEX27)
        eng.set_connectivity_ragged(1, 5, np.array([0, 3, 5], dtype=np.uint64), np.array([0, 1, 2, 3, 4], dtype=np.uint64))
        assert lib.fh_degree_elevation_mesh(eng._h, None, None) == FH_INVALID_STATE
    finally:
        eng.close()
        other.close()


@pytest.mark.gpu
def test_elevation_refinement_and_coarsening_are_held_side_by_side():
    lib = _ffi.lib()
    eng, quadratic = fa.Engine(0), fa.Engine(0)
    try:
        lin = MESHES["hex8_2x2x2_permuted"]()
        eng.set_mesh(lin)
        eng.refine_uniformly()
        fine, ft = eng.refinement()
        eng.elevate_degree(fa.HEX27)                          # leaves the refinement
        high, t = eng.degree_elevation()
        again, ft2 = eng.refinement()
        assert np.array_equal(again.connectivity, fine.connectivity) and np.array_equal(bits(again.vertices), bits(fine.vertices))
        assert np.array_equal(ft2.indices, ft.indices)
        eng.refine_uniformly()                                # leaves the elevation
        high2, t2 = eng.degree_elevation()
        assert np.array_equal(high2.connectivity, high.connectivity) and np.array_equal(bits(high2.vertices), bits(high.vertices))
        assert np.array_equal(t2.indices, t.indices)
        assert lib.fh_degree_coarsening_mesh(eng._h, None, None, None) == FH_INVALID_STATE
        # a quadratic context with a coarsening: a refused elevation leaves it, and the elevation's readers see nothing
        quadratic.set_mesh_from_degree_elevation(eng)
        assert lib.fh_degree_elevation_mesh(eng._h, None, None) == 0          # still held by the linear context
        quadratic.coarsen_degree()
        lin2, _, _ = quadratic.degree_coarsening()
        assert _code(quadratic.elevate_degree, fa.HEX27) == FH_UNSUPPORTED
        _nothing_held(quadratic)
        assert np.array_equal(quadratic.degree_coarsening()[0].connectivity, lin2.connectivity)
        assert lib.fh_refinement_mesh(quadratic._h, None, None) == FH_INVALID_STATE
        # the elevation of the coarsening's mesh, on the context that holds the coarsening's source
        eng.set_mesh_from_degree_coarsening(quadratic)        # a set_mesh: drops what eng held
        _nothing_held(eng)
        assert lib.fh_refinement_mesh(eng._h, None, None) == FH_INVALID_STATE
        eng.elevate_degree(fa.HEX27)
        assert np.array_equal(eng.degree_elevation()[0].connectivity, fa.hex27_mesh_from_hex8(lin2).connectivity)
        assert lib.fh_degree_coarsening_mesh(quadratic._h, None, None, None) == 0
    finally:
        eng.close()
        quadratic.close()


# ---- 7. without a GPU --------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "fenris_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    rust = open(os.path.join(ROOT, "bindings", "fenris_hip_sys.rs")).read()
    lib = _ffi.lib()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert re.search(r"\bpub fn " + name + r"\s*\(", rust), name
        assert getattr(lib, name) is not None
    for name in ("elevate_degree", "elevate_degree_with_transfer", "degree_hierarchy_from_linear"):
        assert callable(getattr(fa, name))
    for name in ("elevate_degree", "degree_elevation", "set_mesh_from_degree_elevation"):
        assert callable(getattr(fa.Engine, name))


def test_the_table_transfer_restates_the_host_converters():
    """the checker itself, on the CPU: every non-vertex node of a host-converted mesh lies at P times the linear vertices"""
    for name, to_kind in (("hex8_3x2x1_permuted", fa.HEX27), ("tet4_bcc1", fa.TET10), ("quad4_3x2_unused", fa.QUAD9), ("tri3_3x2", fa.TRI6)):
        lin = MESHES[name]()
        high = HOST[to_kind](lin)
        off, idx, w = table_transfer(lin, high)
        P = sp.csr_matrix((w, idx.astype(np.int64), off.astype(np.int64)), shape=(high.num_nodes(), lin.num_nodes()))
        assert np.abs(P @ lin.vertices - high.vertices).max() <= 4 * EPS * np.abs(lin.vertices).max()
