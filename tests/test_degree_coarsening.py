"""Degree coarsening on the device (fh_coarsen_degree, Engine.coarsen_degree, coarsen_degree_with_transfer) for Tet10, Tri6, Quad9, Hex20
and Hex27: bit-identical to a sequential sweep that restates the convention of include/fenris_hip.h, the weights against the oracle's
linear basis functions, the device-to-device path, the validation errors, and the Python helpers of fenris_amd.degree."""
import os

import numpy as np
import pytest

import fenris_amd as fa
from fenris_amd import _ffi, quadrature
from oracle import oracle

FH_BAD_ARGUMENT, FH_INVALID_STATE, FH_UNSUPPORTED = 2, 5, 6
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")

_HEX_EDGES = ((0, 1), (0, 3), (0, 4), (1, 2), (1, 5), (2, 3), (2, 6), (3, 7), (4, 5), (4, 7), (5, 6), (6, 7))
_HEX_FACES = ((0, 1, 2, 3), (0, 1, 4, 5), (0, 3, 4, 7), (1, 2, 5, 6), (2, 3, 6, 7), (4, 5, 6, 7))
# kind -> (linear kind, vertex slots, parents of the other local nodes as local nodes)
TABLES = {
    fa.TET10: (fa.TET4, 4, ((0, 1), (1, 2), (0, 2), (0, 3), (2, 3), (1, 3))),
    fa.TRI6: (fa.TRI3, 3, ((0, 1), (1, 2), (0, 2))),
    fa.QUAD9: (fa.QUAD4, 4, ((0, 1), (1, 2), (2, 3), (0, 3), (0, 1, 2, 3))),
    fa.HEX20: (fa.HEX8, 8, _HEX_EDGES),
    fa.HEX27: (fa.HEX8, 8, _HEX_EDGES + _HEX_FACES + (tuple(range(8)),)),
}
ORACLE_KIND = {fa.TET4: oracle.TET4, fa.TRI3: oracle.TRI3, fa.QUAD4: oracle.QUAD4, fa.HEX8: oracle.HEX8}


def sweep(mesh):
    """the convention, sequentially: (linear kind, vertices, connectivity, vertex_nodes, offsets, indices, weights)"""
    linear, nv, parents = TABLES[mesh.elem_kind]
    cells = mesh.connectivity.astype(np.int64).tolist()
    N = mesh.num_nodes()
    is_vertex = [False] * N
    for cell in cells:
        for a in range(nv):
            is_vertex[cell[a]] = True
    vertex_nodes = [i for i in range(N) if is_vertex[i]]
    coarse = {i: j for j, i in enumerate(vertex_nodes)}
    rows = {i: (coarse[i],) for i in vertex_nodes}
    for cell in cells:
        for l, par in enumerate(parents):
            rows.setdefault(cell[nv + l], tuple(sorted(coarse[cell[a]] for a in par)))
    off, idx, w = [0], [], []
    for i in range(N):
        idx += rows[i]
        w += [1.0 / len(rows[i])] * len(rows[i])
        off.append(len(idx))
    conn = [[coarse[cell[a]] for a in range(nv)] for cell in cells]
    return (linear, mesh.vertices[vertex_nodes], np.array(conn, dtype=np.uint64).reshape(-1, nv), np.array(vertex_nodes, dtype=np.uint64),
            np.array(off, dtype=np.uint64), np.array(idx, dtype=np.uint64), np.array(w, dtype=np.float64))


def assert_identical(mesh, lin, t, vertex_nodes):
    kind, v, c, vn, off, idx, w = sweep(mesh)
    assert lin.elem_kind == kind and t.num_coarse == len(vn) and t.num_fine == mesh.num_nodes()
    assert np.array_equal(lin.vertices, v) and np.array_equal(lin.connectivity, c) and np.array_equal(vertex_nodes, vn)
    assert np.array_equal(t.offsets, off) and np.array_equal(t.indices, idx) and np.array_equal(t.weights, w)


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
def permuted(mesh, seed):
    rng = np.random.default_rng(seed)
    perm = rng.permutation(mesh.num_nodes())           # new -> old
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    return fa.Mesh(mesh.vertices[perm], inv[mesh.connectivity.astype(np.int64)].astype(np.uint64), mesh.elem_kind)


def perturbed(mesh, amp, seed):
    rng = np.random.default_rng(seed)
    return fa.Mesh(mesh.vertices + amp * rng.uniform(-1.0, 1.0, mesh.vertices.shape), mesh.connectivity, mesh.elem_kind)


def hex_box():
    return perturbed(fa.procedural.create_rectangular_uniform_hex_mesh(1.0, 5, 4, 3, 1), 0.1, 3)


def golden_json(name, kind):
    import json

    m = json.load(open(os.path.join(GOLDEN, name + ".json")))
    return fa.Mesh(np.array(m["vertices"], dtype=np.float64), np.array(m["connectivity"], dtype=np.uint64), kind)


CONVERTED = {
    "tet10_bcc2": lambda: fa.tet10_mesh_from_tet4(fa.procedural.create_unit_box_uniform_tet_mesh_3d(2)),
    "hex20_5x4x3": lambda: fa.hex20_mesh_from_hex8(hex_box()),
    "hex27_5x4x3": lambda: fa.hex27_mesh_from_hex8(hex_box()),
    "quad9_3x2": lambda: fa.quad9_mesh_from_quad4(perturbed(fa.procedural.create_rectangular_uniform_quad_mesh_2d(1.0, 3, 2, 1, np.array([0.0, 2.0])), 0.05, 5)),
    "tri6_rectangle": lambda: fa.tri6_mesh_from_tri3(golden_json("rectangle_tri3_110", fa.TRI3)),
}
# the linear reference elements: a converted one-cell mesh on them has its nodes at the reference positions
REFERENCE_CELL = {
    fa.TET10: lambda: fa.tet10_mesh_from_tet4(fa.Mesh(np.array([[-1.0, -1, -1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]]), np.array([[0, 1, 2, 3]], dtype=np.uint64), fa.TET4)),
    fa.TRI6: lambda: fa.tri6_mesh_from_tri3(fa.Mesh(np.array([[-1.0, -1], [1, -1], [-1, 1]]), np.array([[0, 1, 2]], dtype=np.uint64), fa.TRI3)),
    fa.QUAD9: lambda: fa.quad9_mesh_from_quad4(fa.Mesh(np.array([[-1.0, -1], [1, -1], [1, 1], [-1, 1]]), np.array([[0, 1, 2, 3]], dtype=np.uint64), fa.QUAD4)),
    fa.HEX20: lambda: fa.hex20_mesh_from_hex8(_reference_hex8()),
    fa.HEX27: lambda: fa.hex27_mesh_from_hex8(_reference_hex8()),
}


def _reference_hex8():
    v = np.array([[-1.0, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]])
    return fa.Mesh(v, np.arange(8, dtype=np.uint64).reshape(1, 8), fa.HEX8)


MESHES = {
    **CONVERTED,
    **{name + "_permuted": (lambda f=f, k=k: permuted(f(), 31 + k)) for k, (name, f) in enumerate(sorted(CONVERTED.items()))},
    "one_tet10": lambda: permuted(perturbed(REFERENCE_CELL[fa.TET10](), 0.1, 1), 41),
    "one_tri6": lambda: permuted(perturbed(REFERENCE_CELL[fa.TRI6](), 0.1, 2), 42),
    "one_quad9": lambda: permuted(perturbed(REFERENCE_CELL[fa.QUAD9](), 0.1, 3), 43),
    "one_hex20": lambda: permuted(perturbed(REFERENCE_CELL[fa.HEX20](), 0.1, 4), 44),
    "one_hex27": lambda: permuted(perturbed(REFERENCE_CELL[fa.HEX27](), 0.1, 5), 45),
    # the reference's own files: Gmsh's and the reference's numbering
    "msh_cube_hex27_8": lambda: fa.io.load_msh_from_file(os.path.join(GOLDEN, "msh", "cube_hex27_8.msh"), fa.HEX27),
    "msh_square_tri6_4": lambda: fa.io.load_msh_from_file(os.path.join(GOLDEN, "msh", "square_tri6_4.msh"), fa.TRI6),
    "json_cube_tet10_24": lambda: golden_json("cube_tet10_24", fa.TET10),
}


@pytest.fixture(scope="module")
def engine():
    eng = fa.Engine(0)
    yield eng
    eng.close()


# ---- 1. bit-identical to the sweep -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(MESHES))
def test_bit_identical_to_the_sweep(engine, name):
    mesh = MESHES[name]()
    lin, t, vn = fa.coarsen_degree_with_transfer(mesh, engine)
    assert_identical(mesh, lin, t, vn)
    sizes = engine.coarsen_degree()                       # the same mesh again: the same arrays
    lin2, t2, vn2 = engine.degree_coarsening()
    assert sizes == (lin.num_nodes(), len(t.indices))
    assert np.array_equal(lin2.vertices, lin.vertices) and np.array_equal(lin2.connectivity, lin.connectivity) and np.array_equal(vn2, vn)
    assert np.array_equal(t2.offsets, t.offsets) and np.array_equal(t2.indices, t.indices) and np.array_equal(t2.weights, t.weights)


@pytest.mark.gpu
def test_the_hex27_box_spans_several_workgroups(engine):
    mesh = MESHES["hex27_5x4x3"]()
    assert mesh.num_nodes() == 693 and mesh.num_nodes() % 256 != 0
    lin = fa.coarsen_degree(mesh, engine)
    assert (lin.num_nodes(), lin.num_elements()) == (6 * 5 * 4, 60)


@pytest.mark.gpu
def test_default_engine():
    mesh = MESHES["quad9_3x2_permuted"]()
    assert_identical(mesh, *fa.coarsen_degree_with_transfer(mesh))


def test_the_sweep_restates_the_header_tables():
    """the checker itself, on the CPU: every non-vertex node of a cell on the linear reference element lies at the mean of its parents"""
    for kind, make in REFERENCE_CELL.items():
        mesh = make()
        _, nv, parents = TABLES[kind]
        cell = mesh.connectivity[0].astype(np.int64)
        assert len(cell) == nv + len(parents)
        for l, par in enumerate(parents):
            assert np.array_equal(mesh.vertices[cell[nv + l]], mesh.vertices[cell[list(par)]].mean(axis=0)), (kind, l)


# ---- 2. weights --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(REFERENCE_CELL))
def test_rows_are_the_linear_basis_at_the_reference_positions(engine, kind):
    mesh = REFERENCE_CELL[kind]()
    lin, t, vn = fa.coarsen_degree_with_transfer(mesh, engine)
    nv = TABLES[kind][1]
    ok = ORACLE_KIND[lin.elem_kind]
    slots = lin.connectivity[0].astype(np.int64)          # coarse vertex of local vertex slot a
    for a in range(nv):
        unit = np.zeros(nv)
        unit[a] = 1.0
        assert np.array_equal(oracle.element_basis(ok, lin.vertices[slots[a]]), unit)   # the cell is the reference element
    P = t.to_scipy().toarray()
    others = np.setdiff1d(np.arange(mesh.num_nodes()), vn.astype(np.int64))
    assert len(others) == mesh.num_nodes() - nv > 0
    for i in others:
        phi = oracle.element_basis(ok, mesh.vertices[i])
        assert np.array_equal(P[i][slots], phi), (kind, i)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CONVERTED))
def test_transfer_reproduces_the_coordinates(engine, name):
    mesh = CONVERTED[name]()
    lin, t, vn = fa.coarsen_degree_with_transfer(mesh, engine)
    assert np.abs(t.apply(lin.vertices) - mesh.vertices).max() <= 1e-15 * np.abs(mesh.vertices).max()
    off = t.offsets.astype(np.int64)
    assert set(np.diff(off).tolist()) <= {1, 2, 4, 8}
    inner = np.ones(len(t.indices), dtype=bool)
    inner[off[:-1]] = False
    assert (np.diff(t.indices.astype(np.int64))[inner[1:]] > 0).all()      # parents strictly ascending within a row


# ---- 3. device to device -----------------------------------------------------------------------------------------------------------
def _laplace_matrix(eng, kind):
    """pattern and values, assembled in a fixed order of summation (FH_ASSEMBLE_REPRODUCIBLE): equal meshes give equal bits"""
    w, p = {fa.TET4: lambda: quadrature.total_order.tetrahedron(2), fa.TRI3: lambda: quadrature.total_order.triangle(2),
            fa.QUAD4: lambda: quadrature.tensor.quadrilateral_gauss(2), fa.HEX8: lambda: quadrature.tensor.hexahedron_gauss(2)}[kind]()
    eng.set_operator(_ffi.LAPLACE)
    eng.set_quadrature_uniform(np.asarray(w, dtype=np.float64), np.asarray(p, dtype=np.float64))
    ro, ci = eng.pattern()
    vals = np.zeros(len(ci))
    eng.assemble_matrix(vals, fa.SCATTER_GATHER | fa.ASSEMBLE_REPRODUCIBLE)
    return ro, ci, vals


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tet10_bcc2_permuted", "hex27_5x4x3_permuted", "quad9_3x2", "tri6_rectangle", "hex20_5x4x3"])
def test_set_mesh_from_degree_coarsening_matches_host_arrays(engine, name):
    mesh = MESHES[name]()
    lin, _, _ = fa.coarsen_degree_with_transfer(mesh, engine)      # the engine now holds the coarsening
    a, b = fa.Engine(0), fa.Engine(0)
    try:
        a.set_mesh_from_degree_coarsening(engine)
        assert a.num_nodes() == lin.num_nodes() and a.num_elements() == lin.num_elements()
        b.set_mesh(lin)
        (roa, cia, va), (rob, cib, vb) = _laplace_matrix(a, lin.elem_kind), _laplace_matrix(b, lin.elem_kind)
        assert np.array_equal(roa, rob) and np.array_equal(cia, cib)
        assert np.abs(vb).max() > 0.0 and np.array_equal(va, vb)
        # the coarsening is still held, and the engine can take it itself
        again, _, _ = engine.degree_coarsening()
        assert np.array_equal(again.connectivity, lin.connectivity)
        engine.set_mesh_from_degree_coarsening(engine)
        assert engine.num_nodes() == lin.num_nodes()
        assert _ffi.lib().fh_degree_coarsening_mesh(engine._h, None, None, None) == FH_INVALID_STATE
    finally:
        a.close()
        b.close()


@pytest.mark.gpu
def test_refinement_and_degree_coarsening_are_held_side_by_side(engine):
    """a Hex8 context refines, takes a Hex27 mesh (both results dropped), coarsens; a refinement formed afterwards leaves the coarsening"""
    lib = _ffi.lib()
    mesh = MESHES["one_hex27"]()
    lin, t, vn = fa.coarsen_degree_with_transfer(mesh, engine)
    assert lib.fh_refinement_mesh(engine._h, None, None) == FH_INVALID_STATE        # fh_refinement_* as without the coarsening
    assert lib.fh_degree_coarsening_mesh(engine._h, None, None, None) == 0
    other = fa.Engine(0)
    try:
        other.set_mesh(lin)
        other.refine_uniformly()
        other_fine, _ = other.refinement()
        assert lib.fh_degree_coarsening_transfer(other._h, None, None, None) == FH_INVALID_STATE
        other.set_mesh_from_degree_coarsening(engine)      # a set_mesh: drops the refinement `other` held
        assert lib.fh_refinement_mesh(other._h, None, None) == FH_INVALID_STATE
        other.refine_uniformly()
        again, _ = other.refinement()
        assert np.array_equal(again.connectivity, other_fine.connectivity) and np.array_equal(again.vertices, other_fine.vertices)
    finally:
        other.close()
    assert_identical(mesh, *engine.degree_coarsening())


# ---- 4. errors ---------------------------------------------------------------------------------------------------------------------
def _code(fn, *args):
    with pytest.raises(fa.FenrisError) as e:
        fn(*args)
    return e.value


def _valid_after(engine):
    mesh = MESHES["one_tri6"]()
    assert_identical(mesh, *fa.coarsen_degree_with_transfer(mesh, engine))


@pytest.mark.gpu
def test_unsupported_kinds(engine):
    tet4 = fa.procedural.create_unit_box_uniform_tet_mesh_3d(1)
    for mesh in (tet4, fa.tet20_mesh_from_tet4(tet4)):
        assert _code(fa.coarsen_degree_with_transfer, mesh, engine).code == FH_UNSUPPORTED
        assert _code(fa.coarsen_degree_with_transfer, mesh).code == FH_UNSUPPORTED
        _valid_after(engine)
    engine.set_connectivity_ragged(1, 5, np.array([0, 3, 5], dtype=np.uint64), np.array([0, 1, 2, 3, 4], dtype=np.uint64))
    assert _code(engine.coarsen_degree).code == FH_UNSUPPORTED
    assert _ffi.lib().fh_degree_coarsening_mesh(engine._h, None, None, None) == FH_INVALID_STATE
    _valid_after(engine)


@pytest.mark.gpu
def test_accessors_without_a_result():
    lib = _ffi.lib()
    eng, other = fa.Engine(0), fa.Engine(0)
    try:
        def nothing_held():
            assert lib.fh_degree_coarsening_mesh(eng._h, None, None, None) == FH_INVALID_STATE
            assert lib.fh_degree_coarsening_transfer(eng._h, None, None, None) == FH_INVALID_STATE
            assert _code(eng.degree_coarsening).code == FH_INVALID_STATE
            assert _code(other.set_mesh_from_degree_coarsening, eng).code == FH_INVALID_STATE

        nothing_held()
        mesh = MESHES["one_quad9"]()
        eng.set_mesh(mesh)
        nothing_held()
        eng.coarsen_degree()
        assert lib.fh_degree_coarsening_mesh(eng._h, None, None, None) == 0
        eng.set_mesh(mesh)
        nothing_held()
    finally:
        eng.close()
        other.close()


_TRI6_V = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [0.5, 0.0], [0.5, 0.5], [0.0, 0.5], [1.0, 1.0], [0.75, 0.0], [1.0, 0.5], [0.75, 0.5]])
BAD = {
    # node 3 is the mid-side node (0, 1) of the first cell and the first vertex of the second
    "vertex_here_midside_there": (fa.Mesh(_TRI6_V, np.array([[0, 1, 2, 3, 4, 5], [3, 1, 6, 7, 8, 9]], dtype=np.uint64), fa.TRI6), "node 3 "),
    # node 4 lies between 1 and 2 in the first cell and between 1 and 6 in the second
    "midside_between_other_vertices": (fa.Mesh(_TRI6_V[:9], np.array([[0, 1, 2, 3, 4, 5], [1, 6, 2, 4, 7, 8]], dtype=np.uint64), fa.TRI6), "node 4 "),
    "node_of_no_cell": (fa.Mesh(_TRI6_V[:7], np.array([[0, 1, 2, 3, 4, 5]], dtype=np.uint64), fa.TRI6), "node 6 "),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(BAD))
def test_invalid_meshes_are_refused(engine, name):
    mesh, names_node = BAD[name]
    err = _code(fa.coarsen_degree_with_transfer, mesh, engine)
    assert err.code == FH_BAD_ARGUMENT and names_node in err.message
    assert _ffi.lib().fh_degree_coarsening_mesh(engine._h, None, None, None) == FH_INVALID_STATE
    _valid_after(engine)


# ---- 5. the helpers ----------------------------------------------------------------------------------------------------------------
def test_matching_vertex_permutation():
    """no GPU: read off the connectivities"""
    old = fa.procedural.create_unit_box_uniform_hex_mesh_3d(2)
    rng = np.random.default_rng(7)
    perm = rng.permutation(old.num_nodes())                # new -> old
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    new = fa.Mesh(old.vertices[perm], inv[old.connectivity.astype(np.int64)].astype(np.uint64), old.elem_kind)
    got = fa.matching_vertex_permutation(new, old)
    assert np.array_equal(got.astype(np.int64), perm)
    assert np.array_equal(fa.matching_vertex_permutation(old, old).astype(np.int64), np.arange(old.num_nodes()))
    rotated = new.connectivity.copy()
    rotated[3] = rotated[3][[1, 2, 3, 0, 5, 6, 7, 4]]
    with pytest.raises(ValueError):
        fa.matching_vertex_permutation(fa.Mesh(new.vertices, rotated, new.elem_kind), old)
    moved = new.vertices.copy()
    moved[5, 1] += 1e-6
    with pytest.raises(ValueError):
        fa.matching_vertex_permutation(fa.Mesh(moved, new.connectivity, new.elem_kind), old)
    with pytest.raises(ValueError):
        fa.matching_vertex_permutation(new, fa.procedural.create_unit_box_uniform_hex_mesh_3d(1))


@pytest.mark.gpu
def test_degree_hierarchy(engine):
    linear, ts = fa.refine_uniformly_repeat_with_transfers(fa.procedural.create_unit_box_uniform_hex_mesh_3d(2), 1, engine)
    high = fa.hex27_mesh_from_hex8(linear[-1])
    coarse, transfers = fa.degree_hierarchy(high, linear, ts, engine)
    assert [m.elem_kind for m in coarse] == [fa.HEX8, fa.HEX8] and [m.num_elements() for m in coarse] == [8, 64]
    assert len(transfers) == 2 and transfers[1].num_fine == high.num_nodes() == 729
    assert coarse[0] is linear[0]
    x = coarse[0].vertices
    for m, t in zip(coarse[1:] + [high], transfers):
        assert t.num_coarse == len(x)
        x = t.apply(x)
        assert np.abs(x - m.vertices).max() <= 1e-15
    # one linear mesh: two levels
    coarse2, transfers2 = fa.degree_hierarchy(high, linear[-1:], [], engine)
    assert len(coarse2) == len(transfers2) == 1 and np.array_equal(coarse2[0].connectivity, coarse[1].connectivity)
    with pytest.raises(ValueError):
        fa.degree_hierarchy(high, linear, [], engine)
