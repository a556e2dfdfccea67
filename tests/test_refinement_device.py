"""Uniform refinement on the device (fh_refine_uniform, Engine.refine_uniformly, refine_uniformly_with_transfer(mesh, engine)) for Tet4,
Tri3, Quad4 and Hex8: bit-identical to a sequential dict sweep that restates the numbering convention of include/fenris_hip.h (for Hex8:
to fh_refine_hex8_uniform), the corner cases of the sort / bucket walk / scan, geometry of the children, the transfer, the
device-to-device path, and Tri3 against the reference's own snapshots."""
import json
import os

import numpy as np
import pytest

import fenris_amd as fa
from fenris_amd import _ffi, quadrature
from oracle import oracle

FH_INVALID_STATE, FH_UNSUPPORTED = 5, 6
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")

# kind -> (parents of the new points as local nodes, children as local indices; n + p names new point p)
TABLES = {
    fa.TET4: (((0, 1), (1, 2), (0, 2), (0, 3), (2, 3), (1, 3)),
              ((0, 4, 6, 7), (4, 1, 5, 9), (6, 5, 2, 8), (7, 9, 8, 3), (4, 6, 7, 9), (4, 9, 5, 6), (6, 7, 9, 8), (6, 8, 9, 5))),
    fa.TRI3: (((0, 1), (1, 2), (2, 0)), ((0, 3, 5), (3, 1, 4), (5, 4, 2), (3, 4, 5))),
    fa.QUAD4: (((0, 1), (1, 2), (2, 3), (3, 0), (0, 1, 2, 3)), ((0, 4, 8, 7), (4, 1, 5, 8), (8, 5, 2, 6), (7, 8, 6, 3))),
}


def sweep(mesh):
    """the convention, sequentially: (vertices, connectivity, offsets, indices, weights)"""
    if mesh.elem_kind == fa.HEX8:
        fine, t = fa.refine_uniformly_with_transfer(mesh)   # no engine: the host sweep fh_refine_hex8_uniform
        return fine.vertices, fine.connectivity, t.offsets, t.indices, t.weights
    points, children = TABLES[mesh.elem_kind]
    v, N = mesh.vertices, mesh.num_nodes()
    label, parents, conn = {}, [], []
    for cell in mesh.connectivity.astype(np.int64).tolist():
        loc = list(cell)
        for par in points:
            key = tuple(sorted(cell[a] for a in par))
            if key not in label:
                label[key] = N + len(parents)
                parents.append(key)
            loc.append(label[key])
        conn += [[loc[i] for i in ch] for ch in children]
    new_v = np.zeros((len(parents), v.shape[1]))
    for m, key in enumerate(parents):
        s = np.zeros(v.shape[1])
        for q in key:
            s = s + v[q]
        new_v[m] = s * (1.0 / len(key))
    counts = np.array([1] * N + [len(k) for k in parents], dtype=np.uint64)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    idx = np.array(list(range(N)) + [q for k in parents for q in k], dtype=np.uint64)
    w = np.concatenate([np.ones(N), np.repeat([1.0 / len(k) for k in parents], [len(k) for k in parents])])
    return (np.concatenate([v, new_v]), np.array(conn, dtype=np.uint64).reshape(-1, mesh.connectivity.shape[1]), off, idx,
            w.astype(np.float64))


def assert_identical(mesh, fine, t):
    v, c, off, idx, w = sweep(mesh)
    assert fine.elem_kind == mesh.elem_kind and t.num_coarse == mesh.num_nodes()
    assert np.array_equal(fine.connectivity, c)
    assert np.array_equal(fine.vertices, v)
    assert np.array_equal(t.offsets, off) and np.array_equal(t.indices, idx) and np.array_equal(t.weights, w)


# ---- meshes ------------------------------------------------------------------------------------------------------------------------
def permuted(mesh, seed):
    rng = np.random.default_rng(seed)
    perm = rng.permutation(mesh.num_nodes())           # new -> old
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    conn = inv[mesh.connectivity.astype(np.int64)][rng.permutation(mesh.num_elements())]
    return fa.Mesh(mesh.vertices[perm], conn.astype(np.uint64), mesh.elem_kind)


def perturbed(mesh, amp, seed):
    rng = np.random.default_rng(seed)
    return fa.Mesh(mesh.vertices + amp * rng.uniform(-1.0, 1.0, mesh.vertices.shape), mesh.connectivity, mesh.elem_kind)


def bcc(n):
    return fa.procedural.create_unit_box_uniform_tet_mesh_3d(n)


def hex_box(n):
    return perturbed(fa.procedural.create_unit_box_uniform_hex_mesh_3d(n), 0.15 / n, 3)


def quad3():
    return perturbed(fa.procedural.create_unit_square_uniform_quad_mesh_2d(3), 0.05, 5)


def tri_reference():
    """tests/unit_tests/mesh/refinement.rs:11-24"""
    v = [[0.0, 0.0], [1.0, 0.0], [2.0, -1.0], [2.5, 1.5], [1.2, 1.0], [0.0, 1.3]]
    return fa.Mesh(np.array(v), np.array([[0, 1, 5], [1, 2, 3], [3, 4, 1], [1, 4, 5]], dtype=np.uint64), fa.TRI3)


def sphere():
    return fa.io.load_msh_from_file(os.path.join(GOLDEN, "msh", "sphere_tet4_593.msh"), fa.TET4)


def tet_fan(k):
    """k tetrahedra (A, B, R_i, R_i+1) around the edge A-B, as tests/test_high_valence.py builds them"""
    ang = np.linspace(0.0, 2.0 * np.pi, k, endpoint=False)
    ring = np.stack([np.cos(ang) * (1.0 + 0.1 * np.sin(3 * ang)), np.sin(ang), np.full(k, 0.5)], axis=1)
    v = np.concatenate([[[0.0, 0.0, 0.0], [0.0, 0.0, 1.0]], ring])
    return fa.Mesh(v, np.array([[0, 1, 2 + i, 2 + (i + 1) % k] for i in range(k)], dtype=np.uint64), fa.TET4)


def padded(mesh, front, back):
    """`front` / `back` vertices that no cell uses in front of / behind the mesh's own"""
    d = mesh.vertices.shape[1]
    v = np.concatenate([np.full((front, d), 7.5), mesh.vertices, np.full((back, d), -3.25)])
    return fa.Mesh(v, mesh.connectivity + np.uint64(front), mesh.elem_kind)


ONE_CELL = {
    "tet4": lambda: fa.Mesh(np.array([[0.1, 0.0, 0.0], [1.0, 0.2, 0.0], [0.0, 1.1, 0.3], [0.2, 0.1, 0.9]]), np.array([[0, 1, 2, 3]], dtype=np.uint64), fa.TET4),
    "tri3": lambda: fa.Mesh(np.array([[0.0, 0.0], [1.0, 0.1], [0.3, 0.9]]), np.array([[2, 0, 1]], dtype=np.uint64), fa.TRI3),
    "quad4": lambda: fa.Mesh(np.array([[0.0, 0.0], [1.0, 0.1], [1.2, 0.9], [-0.1, 1.0]]), np.array([[0, 1, 2, 3]], dtype=np.uint64), fa.QUAD4),
    "hex8": lambda: hex_box(1),
}

MESHES = {
    "tet4_bcc1": lambda: bcc(1), "tet4_bcc2": lambda: bcc(2),
    "tet4_bcc1_permuted": lambda: permuted(bcc(1), 11), "tet4_bcc2_permuted": lambda: permuted(bcc(2), 12),
    "tet4_sphere": sphere, "tri3_reference": tri_reference, "quad4_3x3": quad3,
    "hex8_2": lambda: hex_box(2), "hex8_3": lambda: hex_box(3),
    "hex8_2_permuted": lambda: permuted(hex_box(2), 13), "hex8_3_permuted": lambda: permuted(hex_box(3), 14),
}

CORNER = {
    **{"one_" + k: f for k, f in ONE_CELL.items()},
    "unused_vertices": lambda: padded(bcc(1), 2, 3),
    "fan_of_200": lambda: tet_fan(200),
    # the cells of each pair share vertex 0 and nothing else
    "tets_sharing_a_vertex": lambda: fa.Mesh(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [-1, 0, 0], [0, -1, 0], [0, 0, -1.0]]),
                                             np.array([[0, 1, 2, 3], [0, 5, 4, 6]], dtype=np.uint64), fa.TET4),
    "quads_sharing_a_vertex": lambda: fa.Mesh(np.array([[0, 0], [1, 0], [1, 1], [0, 1], [-1, 0], [-1, -1], [0, -1.0]]),
                                              np.array([[0, 1, 2, 3], [0, 4, 5, 6]], dtype=np.uint64), fa.QUAD4),
    # N around a power of two: bcc(2) has 35 vertices (key width 6); padded to 64 (the largest index fills 6 bits), 65 and 33 (7 and 6
    # bits, one above the power), the numbering mixed so that the cells use the high indices
    "n_35": lambda: bcc(2),
    "n_64": lambda: permuted(padded(bcc(2), 0, 29), 21),
    "n_65": lambda: permuted(padded(bcc(2), 0, 30), 22),
    "n_33_quads_and_centres": lambda: permuted(padded(quad3(), 0, 17), 23),
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
    fine, t = fa.refine_uniformly_with_transfer(mesh, engine)
    assert fine.num_elements() == mesh.num_elements() * len(TABLES.get(mesh.elem_kind, [0, range(8)])[1])
    assert_identical(mesh, fine, t)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tet4_bcc2_permuted", "tri3_reference"])
def test_two_successive_refinements(engine, name):
    meshes, ts = fa.refine_uniformly_repeat_with_transfers(MESHES[name](), 2, engine)
    for k in range(2):
        assert_identical(meshes[k], meshes[k + 1], ts[k])


@pytest.mark.gpu
def test_default_engine_for_kinds_without_a_host_path():
    mesh = tri_reference()
    fine, t = fa.refine_uniformly_with_transfer(mesh)
    assert_identical(mesh, fine, t)
    assert fa.refine_uniformly_repeat(mesh, 2).num_elements() == 64


# ---- 2. corner cases -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CORNER))
def test_corner_cases(engine, name):
    mesh = CORNER[name]()
    fine, t = fa.refine_uniformly_with_transfer(mesh, engine)
    assert_identical(mesh, fine, t)


@pytest.mark.gpu
def test_second_refinement_replaces_the_first_and_set_mesh_drops_it(engine):
    a, b = bcc(1), tri_reference()
    engine.set_mesh(a)
    engine.refine_uniformly()
    engine.set_mesh(b)
    lib = _ffi.lib()
    assert lib.fh_refinement_mesh(engine._h, None, None) == FH_INVALID_STATE
    assert lib.fh_refinement_transfer(engine._h, None, None, None) == FH_INVALID_STATE
    other = fa.Engine(0)
    try:
        with pytest.raises(fa.FenrisError) as e:
            other.set_mesh_from_refinement(engine)
        assert e.value.code == FH_INVALID_STATE
        with pytest.raises(fa.FenrisError) as e:
            engine.refinement()
        assert e.value.code == FH_INVALID_STATE
    finally:
        other.close()
    sizes1 = engine.refine_uniformly()
    assert sizes1 == (15, 16, 6 + 2 * 9)
    engine.set_mesh(a)
    engine.refine_uniformly()
    sizes2 = engine.refine_uniformly()          # the same mesh again: replaces the held result
    fine, t = engine.refinement()
    assert sizes2 == (fine.num_nodes(), fine.num_elements(), len(t.indices))
    assert_identical(a, fine, t)


@pytest.mark.gpu
def test_unsupported_kind(engine):
    m27 = fa.hex27_mesh_from_hex8(fa.procedural.create_unit_box_uniform_hex_mesh_3d(1))
    with pytest.raises(fa.FenrisError) as e:
        fa.refine_uniformly_with_transfer(m27, engine)
    assert e.value.code == FH_UNSUPPORTED
    with pytest.raises(fa.FenrisError) as e:
        fa.refine_uniformly_with_transfer(m27)
    assert e.value.code == FH_UNSUPPORTED


# ---- 3. geometry -------------------------------------------------------------------------------------------------------------------
ORACLE_KIND = {fa.QUAD4: oracle.QUAD4, fa.HEX8: oracle.HEX8}


def corner_dets_and_volumes(mesh):
    """(the Jacobian determinant at every corner of every cell (simplices: the one determinant), the cell volumes)"""
    X = mesh.vertices[mesh.connectivity.astype(np.int64)]
    if mesh.elem_kind in (fa.TET4, fa.TRI3):
        d = X.shape[2]
        det = np.linalg.det(X[:, 1:, :] - X[:, :1, :])
        return det[:, None], det / (6.0 if d == 3 else 2.0)
    d = X.shape[2]
    corners = [[-1, -1], [1, -1], [1, 1], [-1, 1]] if d == 2 else [[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]]
    dets = lambda xi: np.linalg.det(np.einsum("ia,eaj->eji", oracle.element_gradients(ORACLE_KIND[mesh.elem_kind], np.array(xi, dtype=float)), X))
    w, p = quadrature.tensor.quadrilateral_gauss(2) if d == 2 else quadrature.tensor.hexahedron_gauss(2)
    vol = sum(wq * dets(xq) for wq, xq in zip(np.asarray(w), np.asarray(p)))
    return np.stack([dets(xi) for xi in corners], axis=1), vol


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tet4_bcc2", "tet4_sphere", "tri3_reference", "quad4_3x3", "hex8_2"])
def test_children_keep_orientation_and_volume(engine, name):
    mesh = MESHES[name]()
    dets, vol = corner_dets_and_volumes(mesh)
    assert (dets > 0).all()                       # positively oriented parents
    fine = fa.refine_uniformly(mesh, engine)
    cdets, cvol = corner_dets_and_volumes(fine)
    assert (cdets > 0).all()
    C = fine.num_elements() // mesh.num_elements()
    per_parent = cvol.reshape(-1, C)
    assert np.abs(per_parent.sum(axis=1) - vol).max() <= 1e-12 * np.abs(vol).max()
    assert abs(cvol.sum() - vol.sum()) <= 1e-12 * vol.sum()
    if mesh.elem_kind == fa.TET4:
        assert np.abs(per_parent - vol[:, None] / 8.0).max() <= 1e-13 * np.abs(vol).max()


@pytest.mark.gpu
def test_tet4_stays_within_three_congruence_classes(engine):
    rng = np.random.default_rng(8)
    mesh = fa.Mesh(rng.uniform(-1.0, 1.0, (4, 3)), np.array([[0, 1, 2, 3]], dtype=np.uint64), fa.TET4)
    if np.linalg.det(mesh.vertices[1:] - mesh.vertices[0]) < 0:
        mesh = fa.Mesh(mesh.vertices[[0, 2, 1, 3]], mesh.connectivity, fa.TET4)
    for level in range(1, 4):
        mesh = fa.refine_uniformly(mesh, engine)
        X = mesh.vertices[mesh.connectivity.astype(np.int64)]
        pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
        lengths = np.stack([np.linalg.norm(X[:, a] - X[:, b], axis=1) for a, b in pairs], axis=1) * 2.0 ** level
        classes = {tuple(r) for r in np.round(np.sort(lengths, axis=1), 6).tolist()}
        assert len(classes) <= 3, (level, len(classes))
    assert mesh.num_elements() == 512


# ---- 4. transfer -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tet4_bcc2_permuted", "tet4_sphere", "tri3_reference", "quad4_3x3", "hex8_2_permuted"])
def test_transfer(engine, name):
    mesh = MESHES[name]()
    fine, t = fa.refine_uniformly_with_transfer(mesh, engine)
    N, d = mesh.num_nodes(), mesh.vertices.shape[1]
    off, idx = t.offsets.astype(np.int64), t.indices.astype(np.int64)
    assert t.num_fine == fine.num_nodes() and off[0] == 0 and off[-1] == len(idx) == len(t.weights)
    assert np.abs(np.add.reduceat(t.weights, off[:-1]) - 1.0).max() <= 1e-15
    inner = np.ones(len(idx), dtype=bool)
    inner[off[:-1]] = False                                  # (not the first entry of a row)
    assert (np.diff(idx)[inner[1:]] > 0).all()               # parents strictly ascending within a row
    assert np.array_equal(off[: N + 1], np.arange(N + 1)) and np.array_equal(idx[:N], np.arange(N)) and (t.weights[:N] == 1.0).all()
    assert set(np.diff(off)[N:].tolist()) <= {2, 4, 8}
    assert np.abs(t.apply(mesh.vertices) - fine.vertices).max() <= 1e-14
    rng = np.random.default_rng(2)
    A, b = rng.standard_normal((d, 2)), rng.standard_normal(2)
    assert np.abs(t.apply(mesh.vertices @ A + b) - (fine.vertices @ A + b)).max() <= 1e-13
    if mesh.elem_kind in ORACLE_KIND:
        # a bi- / trilinear field: the fine value at local index l of parent e is the parent's basis at l's reference point
        field = rng.standard_normal((N, 2))
        via_t = t.apply(field)
        sgn = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]] if d == 2 else
                       [[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], dtype=float)
        C = len(sgn)
        for e in range(mesh.num_elements()):
            cn = mesh.connectivity[e].astype(np.int64)
            for ch in range(C):
                child = fine.connectivity[C * e + ch].astype(np.int64)
                # child ch sits at corner ch of the parent (Quad4: children in the order of the corners; Hex8: (cx, cy, cz) bits)
                origin = sgn[ch] if d == 2 else np.array([ch & 1, (ch >> 1) & 1, (ch >> 2) & 1], dtype=float) * 2.0 - 1.0
                for a in range(C):
                    xi = origin / 2.0 + sgn[a] / 2.0
                    phi = oracle.element_basis(ORACLE_KIND[mesh.elem_kind], xi)
                    assert np.abs(phi @ field[cn] - via_t[child[a]]).max() <= 1e-13
                    assert np.abs(phi @ mesh.vertices[cn] - fine.vertices[child[a]]).max() <= 1e-14


# ---- 5. device to device -----------------------------------------------------------------------------------------------------------
def _residual(eng, kind, num_nodes, seed):
    d = _ffi.ELEM_DIM[kind]
    w, p = {fa.TET4: lambda: quadrature.total_order.tetrahedron(2), fa.TRI3: lambda: quadrature.total_order.triangle(2),
            fa.QUAD4: lambda: quadrature.tensor.quadrilateral_gauss(2), fa.HEX8: lambda: quadrature.tensor.hexahedron_gauss(2)}[kind]()
    w, p = np.asarray(w, dtype=np.float64), np.asarray(p, dtype=np.float64)
    if d == 3:
        lame = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.3))
        eng.set_operator(_ffi.LINEAR_ELASTIC)
        eng.set_quadrature_uniform(w, p, np.tile(np.asarray(lame.as_pair(), dtype=np.float64), (len(w), 1)))
        s = 3
    else:
        eng.set_operator(_ffi.LAPLACE)
        eng.set_quadrature_uniform(w, p)
        s = 1
    u = np.random.default_rng(seed).standard_normal(s * num_nodes)
    eng.set_u(u)
    out = np.zeros(s * num_nodes)
    eng.assemble_vector(out)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tet4_bcc2_permuted", "tri3_reference", "quad4_3x3", "hex8_2_permuted"])
def test_set_mesh_from_refinement_matches_host_arrays(engine, name):
    mesh = MESHES[name]()
    fine, _ = fa.refine_uniformly_with_transfer(mesh, engine)      # the engine now holds the refinement
    a, b = fa.Engine(0), fa.Engine(0)
    try:
        a.set_mesh_from_refinement(engine)
        assert a.num_nodes() == fine.num_nodes() and a.num_elements() == fine.num_elements()
        b.set_mesh(fine)
        ra, rb = _residual(a, mesh.elem_kind, fine.num_nodes(), 4), _residual(b, mesh.elem_kind, fine.num_nodes(), 4)
        assert np.abs(rb).max() > 0.0
        assert np.array_equal(ra, rb)
        # the refinement is still held, and the engine can take it itself
        again, _ = engine.refinement()
        assert np.array_equal(again.connectivity, fine.connectivity)
        engine.set_mesh_from_refinement(engine)
        assert engine.num_nodes() == fine.num_nodes()
        assert _ffi.lib().fh_refinement_mesh(engine._h, None, None) == FH_INVALID_STATE
    finally:
        a.close()
        b.close()


# ---- 8. the default path is unchanged (no GPU) -------------------------------------------------------------------------------------
def test_hex8_without_an_engine_is_the_host_sweep():
    import ctypes as C

    mesh = hex_box(2)
    fine, t = fa.refine_uniformly_with_transfer(mesh)
    lib = _ffi.lib()
    N, E = mesh.num_nodes(), mesh.num_elements()
    nv, nnz = C.c_uint64(), C.c_uint64()
    args = (_ffi.fp(mesh.vertices), N, _ffi.up(mesh.connectivity), E)
    assert lib.fh_refine_hex8_uniform(*args, None, C.byref(nv), None, None, None, None, C.byref(nnz)) == 0
    v, c = np.zeros((nv.value, 3)), np.zeros((8 * E, 8), dtype=np.uint64)
    off, idx, w = np.zeros(nv.value + 1, dtype=np.uint64), np.zeros(nnz.value, dtype=np.uint64), np.zeros(nnz.value)
    assert lib.fh_refine_hex8_uniform(*args, _ffi.fp(v), C.byref(nv), _ffi.up(c), _ffi.up(off), _ffi.up(idx), _ffi.fp(w), C.byref(nnz)) == 0
    assert np.array_equal(fine.vertices, v) and np.array_equal(fine.connectivity, c)
    assert np.array_equal(t.offsets, off) and np.array_equal(t.indices, idx) and np.array_equal(t.weights, w)
    assert fa.refine_uniformly_repeat(mesh, 0) is mesh
    meshes, ts = fa.refine_uniformly_repeat_with_transfers(mesh, 1)
    assert np.array_equal(meshes[1].connectivity, c) and np.array_equal(ts[0].weights, w)


def test_the_sweep_restates_the_header_tables():
    """the checker itself, on the CPU: counts of a one-cell mesh of each kind"""
    for name, (nv, nc) in {"tet4": (10, 8), "tri3": (6, 4), "quad4": (9, 4)}.items():
        v, c, off, idx, w = sweep(ONE_CELL[name]())
        assert (len(v), len(c)) == (nv, nc) and off[-1] == len(idx) == len(w)


# ---- 9. Tri3 against the reference's snapshots -------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_tri3_against_the_reference_snapshots(engine):
    """the reference labels ALL vertices by first appearance, old ones included: match the vertices by their coordinates, then the
    cells must agree in order and in node order"""
    snaps = json.load(open(os.path.join(GOLDEN, "refinement_tri3.json")))["meshes"]
    mesh = tri_reference()
    ours = {"refined0": fa.refine_uniformly_repeat(mesh, 0, engine), "refined1": fa.refine_uniformly_repeat(mesh, 1, engine),
            "refined2": fa.refine_uniformly_repeat(mesh, 2, engine), "refined_once": fa.refine_uniformly(mesh, engine)}
    for name, snap in snaps.items():
        sv, sc = np.array(snap["vertices"]), np.array(snap["cells"], dtype=np.int64)
        m = ours[name]
        assert m.num_nodes() == len(sv) and m.num_elements() == len(sc)
        dist = np.abs(m.vertices[:, None, :] - sv[None, :, :]).max(axis=2)
        to_snap = dist.argmin(axis=1)
        assert dist.min(axis=1).max() <= 1e-12 and len(np.unique(to_snap)) == len(sv)
        assert np.array_equal(to_snap[m.connectivity.astype(np.int64)], sc)
