"""Boundary-face search on the device (fh_find_boundary_faces, fh_boundary_faces / _vertices / _cells; Mesh.find_boundary_*;
Mesh.extract_surface_mesh) against the independent restatement in tests/boundary_reference.py: every index array exactly, order
included.  The CPU tests check the exports and the checker itself against the reference's known answers
(tests/unit_tests/mesh.rs:22-83) and against geometry (outward normals, surface area)."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import boundary_reference as br  # noqa: E402
import fenris_amd as fa  # noqa: E402
from fenris_amd import _ffi  # noqa: E402

P = fa.procedural
MSH = os.path.join(ROOT, "tests", "golden", "msh")
NEW_EXPORTS = ["fh_find_boundary_faces", "fh_boundary_faces", "fh_boundary_faces_dev", "fh_boundary_vertices", "fh_boundary_cells",
               "fh_assemble_surface_load", "fh_assemble_surface_load_dev", "fh_physical_face_quadrature_points",
               "fh_physical_face_quadrature_points_dev"]


# ------------------------------------------------------------------------------------------------------------------- no GPU
def test_new_exports_in_header_ffi_and_bindings():
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "fenris_hip.h")).read(), flags=re.S)
    rs = open(os.path.join(ROOT, "bindings", "fenris_hip_sys.rs")).read()
    lib = _ffi.lib()
    for name in NEW_EXPORTS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _ffi.exported_symbols(), name
        assert "pub fn %s(" % name in rs, name
        assert getattr(lib, name) is not None


def _quad9_two_elements():
    conn = np.array([[0, 1, 4, 5, 6, 10, 13, 12, 11], [1, 2, 3, 4, 7, 8, 14, 10, 9]], dtype=np.uint64)
    verts = np.array([[0, 0], [1, 0], [2, 0], [0, 1], [1, 1], [0, 1], [.5, 0], [1.5, 0], [2, .5], [1.5, .5], [1, .5], [.5, .5], [0, .5],
                      [.5, 1], [1.5, 1]], dtype=np.float64)
    return fa.Mesh(verts, conn, fa.QUAD9)


def test_checker_reproduces_the_known_answers_of_the_reference():
    # tests/unit_tests/mesh.rs:22-43
    m = P.create_unit_square_uniform_quad_mesh_2d(1)
    _, cells, lfs = br.find_boundary_faces(br.QUAD4, m.connectivity)
    assert cells.tolist() == [0, 0, 0, 0] and sorted(lfs.tolist()) == [0, 1, 2, 3]
    # :46-53
    m9 = fa.quad9_mesh_from_quad4(m)
    assert br.find_boundary_vertices(br.QUAD9, m9.connectivity).tolist() == [0, 1, 2, 3, 4, 5, 6, 7]
    # :55-82
    assert br.find_boundary_vertices(br.QUAD9, _quad9_two_elements().connectivity).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13, 14]


@pytest.mark.parametrize("name", ["hex", "tet", "quad", "tri", "hex27", "tet10", "quad9", "tri6", "hex20"])
def test_checker_faces_point_outward_and_cover_the_box(name):
    m = _structured(name, 3)
    _, cells, lfs = br.find_boundary_faces(m.elem_kind, m.connectivity)
    A, cf, cc = br.face_area_vectors(m.elem_kind, m.vertices, m.connectivity, cells, lfs)
    assert np.all(np.sum((cf - cc) * A, axis=1) > 0)          # (centroid of face - centroid of cell) . a
    d = m.vertices.shape[1]
    assert abs(float(np.sum(np.sqrt(np.sum(A * A, axis=1)))) - (6.0 if d == 3 else 4.0)) < 1e-13
    assert np.abs(A.sum(axis=0)).max() < 1e-14               # closed surface


def test_checker_tet_closed_forms_up_to_6():
    """BCC box of resolution n (procedural.rs:286-403): 12 n^2 boundary faces and cells, 6 n^2 + 2 boundary vertices"""
    for n in range(1, 7):
        m = P.create_unit_box_uniform_tet_mesh_3d(n)
        fn, cells, _ = br.find_boundary_faces(br.TET4, m.connectivity)
        assert (len(cells), len(np.unique(fn)), len(np.unique(cells))) == (12 * n * n, 6 * n * n + 2, 12 * n * n)


# ---------------------------------------------------------------------------------------------------------------- mesh zoo
def _structured(name, n):
    if name == "hex":
        return P.create_unit_box_uniform_hex_mesh_3d(n)
    if name == "tet":
        return P.create_unit_box_uniform_tet_mesh_3d(n)
    if name == "quad":
        return P.create_unit_square_uniform_quad_mesh_2d(n)
    if name == "tri":
        return P.create_unit_square_uniform_tri_mesh_2d(n)
    if name == "hex27":
        return fa.hex27_mesh_from_hex8(_structured("hex", n))
    if name == "hex20":
        return fa.hex20_mesh_from_hex8(_structured("hex", n))
    if name == "tet10":
        return fa.tet10_mesh_from_tet4(_structured("tet", n))
    if name == "tet20":
        return fa.tet20_mesh_from_tet4(_structured("tet", n))
    if name == "quad9":
        return fa.quad9_mesh_from_quad4(_structured("quad", n))
    if name == "tri6":
        return fa.tri6_mesh_from_tri3(_structured("tri", n))
    raise KeyError(name)


def _permuted(m, seed):
    rng = np.random.default_rng(seed)
    vp = rng.permutation(m.num_nodes())
    inv = np.empty_like(vp)
    inv[vp] = np.arange(len(vp))
    conn = inv[m.connectivity.astype(np.int64)][rng.permutation(m.num_elements())].astype(np.uint64)
    return fa.Mesh(m.vertices[vp], conn, m.elem_kind)


def _check_against_checker(m, engine=None):
    eng = engine or fa.Engine()
    eng.set_mesh(m)
    fn, cells, lfs = eng.find_boundary_faces()
    rfn, rcells, rlfs = br.find_boundary_faces(m.elem_kind, m.connectivity)
    assert fn.shape[0] == len(rcells)
    if len(rcells):
        assert np.array_equal(fn, rfn)
    assert np.array_equal(cells, rcells) and np.array_equal(lfs, rlfs)
    assert cells.dtype == np.uint64 and lfs.dtype == np.uint32 and fn.dtype == np.uint64
    assert np.array_equal(eng.boundary_vertices(), br.find_boundary_vertices(m.elem_kind, m.connectivity))
    assert np.array_equal(eng.boundary_cells(), br.find_boundary_cells(m.elem_kind, m.connectivity))
    return fn, cells, lfs


# --------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_known_answers_through_the_c_abi():
    eng = fa.Engine()
    m = P.create_unit_square_uniform_quad_mesh_2d(1)
    eng.set_mesh(m)
    _, cells, lfs = eng.find_boundary_faces()
    assert cells.tolist() == [0, 0, 0, 0] and sorted(lfs.tolist()) == [0, 1, 2, 3]
    eng.set_mesh(fa.quad9_mesh_from_quad4(m))
    assert eng.boundary_vertices().tolist() == [0, 1, 2, 3, 4, 5, 6, 7]
    eng.set_mesh(_quad9_two_elements())
    assert eng.boundary_vertices().tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 12, 13, 14]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hex", "tet", "quad", "tri", "hex27", "tet10", "quad9", "tri6", "hex20"])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_structured_meshes_every_kind(name, n):
    _check_against_checker(_structured(name, n))


@pytest.mark.gpu
def test_tet20_has_no_faces():
    m = _structured("tet20", 2)
    eng = fa.Engine()
    eng.set_mesh(m)
    fn, cells, lfs = eng.find_boundary_faces()
    assert len(cells) == 0 and len(lfs) == 0 and fn.shape[0] == 0
    assert len(eng.boundary_vertices()) == 0 and len(eng.boundary_cells()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hex", "tet", "quad", "tri", "hex27", "tet10", "quad9", "tri6", "hex20"])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_permuted_numbering(name, seed):
    _check_against_checker(_permuted(_structured(name, 4), seed))


@pytest.mark.gpu
@pytest.mark.parametrize("fname,kind", [("cube_hex27_8.msh", fa.HEX27), ("cube_hex8_8.msh", fa.HEX8), ("rectangle_tri3_110.msh", fa.TRI3),
                                        ("square_tri6_4.msh", fa.TRI6), ("square_quad9_4.msh", fa.QUAD9), ("square_tri3_4.msh", fa.TRI3),
                                        ("cube_tet4_24.msh", fa.TET4), ("sphere_tet4_593.msh", fa.TET4), ("cube_tet10_24.msh", fa.TET10),
                                        ("square_quad4_4.msh", fa.QUAD4), ("square_quad4_79.msh", fa.QUAD4)])
def test_golden_msh_meshes(fname, kind):
    m = fa.io.load_msh_from_file(os.path.join(MSH, fname), kind)
    _, cells, _ = _check_against_checker(m)
    assert len(cells) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hex", "tet", "hex27"])
def test_mesh_with_an_interior_void(name):
    m = _structured(name, 5)
    corners = br.CELL_CORNERS[m.elem_kind]
    c = m.vertices[m.connectivity[:, :corners].astype(np.int64)].mean(axis=1)
    keep = np.abs(c - 0.5).max(axis=1) > 0.1 + 1e-9        # drop the middle cell(s)
    assert 0 < keep.sum() < len(keep)
    mv = fa.Mesh(m.vertices, m.connectivity[keep], m.elem_kind)
    fn, _, _ = _check_against_checker(mv)
    full = br.find_boundary_faces(m.elem_kind, m.connectivity)[0]
    assert len(fn) > len(full)                              # the void's wall is boundary too


@pytest.mark.gpu
def test_three_cells_on_one_face_is_not_boundary():
    # three tetrahedra over the triangle (0, 1, 2): the shared face occurs three times -- not a boundary face (count != 1)
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, -1], [1, 1, 1]], dtype=np.float64)
    conn = np.array([[0, 1, 2, 3], [0, 2, 1, 4], [0, 1, 2, 5]], dtype=np.uint64)
    m = fa.Mesh(verts, conn, fa.TET4)
    fn, _, _ = _check_against_checker(m)
    assert len(fn) == 9 and not any(sorted(f) == [0, 1, 2] for f in fn.tolist())
    # and in 2D: three quadrilaterals on one edge
    v2 = np.array([[0, 0], [1, 0], [1, 1], [0, 1], [2, 0], [2, 1], [1, 2], [0, 2]], dtype=np.float64)
    c2 = np.array([[0, 1, 2, 3], [1, 4, 5, 2], [1, 2, 6, 7]], dtype=np.uint64)
    fn2, _, _ = _check_against_checker(fa.Mesh(v2, c2, fa.QUAD4))
    assert not any(sorted(f) == [1, 2] for f in fn2.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hex", "tet", "quad", "tri", "hex27", "tet10", "quad9", "tri6", "hex20"])
def test_one_element_mesh(name):
    m = _structured(name, 1)
    m1 = fa.Mesh(m.vertices, m.connectivity[:1], m.elem_kind)
    _, cells, lfs = _check_against_checker(m1)
    assert sorted(lfs.tolist()) == list(range(len(br.FACES[m.elem_kind]))) and set(cells.tolist()) == {0}


@pytest.mark.gpu
def test_states_and_cache():
    eng = fa.Engine()
    lib, h = eng._lib, eng._h
    import ctypes as C

    nf, k = C.c_uint64(7), C.c_uint32(7)
    assert lib.fh_find_boundary_faces(h, C.byref(nf), C.byref(k)) == _ffi.FH_INVALID_STATE
    assert lib.fh_boundary_vertices(h, C.byref(nf), None) == _ffi.FH_INVALID_STATE
    eng.set_connectivity_ragged(1, 4, [0, 2, 4], [0, 1, 2, 3])
    assert lib.fh_find_boundary_faces(h, C.byref(nf), C.byref(k)) == _ffi.FH_UNSUPPORTED
    assert lib.fh_boundary_cells(h, C.byref(nf), None) == _ffi.FH_UNSUPPORTED
    m = _structured("hex", 3)
    fn, cells, lfs = _check_against_checker(m, eng)
    eng.update_vertices(m.vertices * 2.0)                      # keeps the cached result
    fn2, cells2, lfs2 = eng.find_boundary_faces()
    assert np.array_equal(fn, fn2) and np.array_equal(cells, cells2) and np.array_equal(lfs, lfs2)
    _check_against_checker(_structured("tet", 2), eng)         # fh_set_mesh drops it
    # the _dev form gives the same arrays
    import torch

    eng.set_mesh(m)
    F = len(cells)
    fn_t = torch.zeros((F, 4), dtype=torch.int64, device="cuda")
    c_t = torch.zeros(F, dtype=torch.int64, device="cuda")
    l_t = torch.zeros(F, dtype=torch.int32, device="cuda")
    eng._check(lib.fh_find_boundary_faces(h, C.byref(nf), C.byref(k)))
    assert (nf.value, k.value) == (F, 4)
    eng._check(lib.fh_boundary_faces_dev(h, C.c_void_p(fn_t.data_ptr()), C.c_void_p(c_t.data_ptr()), C.c_void_p(l_t.data_ptr())))
    eng._check(lib.fh_synchronize(h))
    assert np.array_equal(fn_t.cpu().numpy().astype(np.uint64), fn) and np.array_equal(c_t.cpu().numpy().astype(np.uint64), cells)
    assert np.array_equal(l_t.cpu().numpy().astype(np.uint32), lfs)


@pytest.mark.gpu
def test_python_mirror_and_surface_mesh():
    m = _permuted(_structured("tet", 3), 5)
    bf = m.find_boundary_faces()
    fn, cells, lfs = bf
    rfn, rcells, rlfs = br.find_boundary_faces(m.elem_kind, m.connectivity)
    assert np.array_equal(fn, rfn) and np.array_equal(cells, rcells) and np.array_equal(lfs, rlfs)
    assert np.array_equal(m.find_boundary_vertices(), np.unique(rfn))
    assert np.array_equal(m.find_boundary_cells(), np.unique(rcells))
    # extract_surface_mesh (mesh.rs:505-516): faces in search order, orientation kept, vertices compacted like keep_cells (:305-354)
    sm = m.extract_surface_mesh()
    keep = np.unique(rfn).astype(np.int64)
    assert sm.face_kind == "Tri3" and np.array_equal(sm.vertices, m.vertices[keep])
    assert np.array_equal(keep[sm.connectivity.astype(np.int64)], rfn.astype(np.int64))
    # select: "the face x = 1" in one line
    right = bf.select(lambda c, n: n[:, 0] > 0.5)
    assert len(right) == 2 * 3 * 3                              # two triangles per cube face
    assert np.allclose(m.vertices[right.vertices().astype(np.int64)][:, 0], 1.0)
    assert np.array_equal(np.sort(right.vertices()), np.flatnonzero(m.vertices[:, 0] == 1.0).astype(np.uint64))
    A, cf, cc = br.face_area_vectors(m.elem_kind, m.vertices, m.connectivity, cells, lfs)
    unit = A / np.sqrt(np.sum(A * A, axis=1, keepdims=True))
    assert np.abs(bf.normals() - unit.astype(np.float64)).max() < 1e-14
    assert np.abs(bf.centroids() - cf.astype(np.float64)).max() < 1e-15


def _boundary_layer_check(m, fn, cells, lfs, on_surface):
    """the checker on the cells that touch the surface only; of its faces those whose nodes all lie on the surface are the mesh's
    boundary faces (an interior face of a box mesh with two or more cells per side has a node off the surface), in the same order"""
    corners = br.CELL_CORNERS[m.elem_kind]
    layer = np.flatnonzero(on_surface[m.connectivity[:, :corners].astype(np.int64)].any(axis=1))
    rfn, rcells, rlfs = br.find_boundary_faces(m.elem_kind, m.connectivity[layer])
    keep = on_surface[rfn.astype(np.int64)].all(axis=1)
    return rfn[keep], layer[rcells[keep].astype(np.int64)].astype(np.uint64), rlfs[keep]


@pytest.mark.gpu
def test_full_size_hex8_216():
    n = 216
    m = P.create_unit_box_uniform_hex_mesh_3d(n)
    eng = fa.Engine()
    eng.set_mesh(m)
    fn, cells, lfs = eng.find_boundary_faces()
    assert len(cells) == 6 * n * n
    bv, bc = eng.boundary_vertices(), eng.boundary_cells()
    assert len(bv) == (n + 1) ** 3 - (n - 1) ** 3 and len(bc) == n ** 3 - (n - 2) ** 3
    on_surface = ((m.vertices == 0.0) | (m.vertices == 1.0)).any(axis=1)
    assert np.array_equal(bv, np.flatnonzero(on_surface).astype(np.uint64))
    rfn, rcells, rlfs = _boundary_layer_check(m, fn, cells, lfs, on_surface)
    assert len(rcells) == 6 * n * n
    stride = 7   # a strided sample of the order, then everything
    assert np.array_equal(fn[::stride], rfn[::stride]) and np.array_equal(cells[::stride], rcells[::stride])
    assert np.array_equal(fn, rfn) and np.array_equal(cells, rcells) and np.array_equal(lfs, rlfs)
    assert np.array_equal(bc, np.unique(rcells))


@pytest.mark.gpu
def test_full_size_c3_tet_mesh():
    """the C3 benchmark mesh: BCC box of resolution 75, vertices and elements permuted (MT19937 seed 12345); closed forms fitted by
    test_checker_tet_closed_forms_up_to_6"""
    n = 75
    m0 = P.create_unit_box_uniform_tet_mesh_3d(n)
    rng = np.random.Generator(np.random.MT19937(12345))
    vp = rng.permutation(m0.num_nodes())
    inv = np.empty_like(vp)
    inv[vp] = np.arange(len(vp))
    m = fa.Mesh(m0.vertices[vp], inv[m0.connectivity.astype(np.int64)][rng.permutation(m0.num_elements())].astype(np.uint64), fa.TET4)
    eng = fa.Engine()
    eng.set_mesh(m)
    fn, cells, lfs = eng.find_boundary_faces()
    bv, bc = eng.boundary_vertices(), eng.boundary_cells()
    assert (len(cells), len(bv), len(bc)) == (12 * n * n, 6 * n * n + 2, 12 * n * n)
    on_surface = ((m.vertices == 0.0) | (m.vertices == 1.0)).any(axis=1)
    assert np.array_equal(bv, np.flatnonzero(on_surface).astype(np.uint64))
    rfn, rcells, rlfs = _boundary_layer_check(m, fn, cells, lfs, on_surface)
    assert np.array_equal(fn[::5], rfn[::5])
    assert np.array_equal(fn, rfn) and np.array_equal(cells, rcells) and np.array_equal(lfs, rlfs)
    assert np.array_equal(bc, np.unique(rcells))
