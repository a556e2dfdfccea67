"""Uniform Hex8 refinement and its transfer (fh_refine_hex8_uniform; refine_uniformly, refine_uniformly_repeat, permute_transfer): counts,
positive Jacobians, volume, partition of unity, exact trilinear interpolation against the oracle's basis, and box(n) -> box(2n)."""
import numpy as np

import fenris_amd as fa
from fenris_amd import quadrature
from oracle import oracle


def _unique_edges_faces(conn):
    edges, faces = set(), set()
    E = ((0, 1), (0, 3), (0, 4), (1, 2), (1, 5), (2, 3), (2, 6), (3, 7), (4, 5), (4, 7), (5, 6), (6, 7))
    F = ((0, 1, 2, 3), (0, 1, 4, 5), (0, 3, 4, 7), (1, 2, 5, 6), (2, 3, 6, 7), (4, 5, 6, 7))
    for c in conn.astype(np.int64):
        edges.update(tuple(sorted((c[a], c[b]))) for a, b in E)
        faces.update(tuple(sorted(c[list(f)])) for f in F)
    return len(edges), len(faces)


def _perturbed(n, seed=3, amp=0.15):
    m = fa.procedural.create_unit_box_uniform_hex_mesh_3d(n)
    rng = np.random.default_rng(seed)
    v = m.vertices + amp / n * rng.uniform(-1.0, 1.0, m.vertices.shape)
    return fa.Mesh(v, m.connectivity, fa.HEX8)


def _jacobian_dets(mesh, points):
    out = []
    for xi in points:
        g = oracle.element_gradients(oracle.HEX8, xi)          # 3 x 8
        X = mesh.vertices[mesh.connectivity.astype(np.int64)]  # E x 8 x 3
        J = np.einsum("ia,eaj->eji", g, X)
        out.append(np.linalg.det(J))
    return np.array(out)


def _volume(mesh):
    w, p = quadrature.tensor.hexahedron_gauss(2)
    return float(np.sum(np.asarray(w)[:, None] * np.abs(_jacobian_dets(mesh, p))))


def test_vertex_count_and_coarse_vertices_first():
    for coarse in (fa.procedural.create_unit_box_uniform_hex_mesh_3d(3), _perturbed(2)):
        fine, t = fa.refine_uniformly_with_transfer(coarse)
        ne, nf = _unique_edges_faces(coarse.connectivity)
        assert fine.num_nodes() == coarse.num_nodes() + ne + nf + coarse.num_elements()
        assert fine.num_elements() == 8 * coarse.num_elements()
        assert np.array_equal(fine.vertices[: coarse.num_nodes()], coarse.vertices)
        nc = coarse.num_nodes()
        assert np.array_equal(t.offsets[: nc + 1], np.arange(nc + 1))
        assert np.array_equal(t.indices[:nc], np.arange(nc)) and np.all(t.weights[:nc] == 1.0)


def test_children_positive_and_volume_preserved():
    w, p = quadrature.tensor.hexahedron_gauss(2)
    for coarse in (fa.procedural.create_rectangular_uniform_hex_mesh(2.0, 1, 2, 1, 2), _perturbed(3)):
        fine = fa.refine_uniformly(coarse)
        assert (_jacobian_dets(fine, p) > 0.0).all()
        assert abs(_volume(fine) - _volume(coarse)) <= 1e-12 * _volume(coarse)
    twice = fa.refine_uniformly_repeat(_perturbed(2), 2)
    assert twice.num_elements() == 64 * 8 and (_jacobian_dets(twice, p) > 0.0).all()


def test_transfer_rows_and_weights():
    fine, t = fa.refine_uniformly_with_transfer(_perturbed(3))
    counts = np.diff(t.offsets.astype(np.int64))
    assert set(np.unique(counts)) == {1, 2, 4, 8}
    for c in (1, 2, 4, 8):
        rows = np.where(counts == c)[0]
        for r in rows[:50]:
            assert np.all(t.weights[t.offsets[r]:t.offsets[r + 1]] == 1.0 / c)
            ids = t.indices[t.offsets[r]:t.offsets[r + 1]]
            assert np.all(np.diff(ids.astype(np.int64)) > 0)
    sums = np.add.reduceat(t.weights, t.offsets[:-1].astype(np.int64))
    assert np.allclose(sums, 1.0, rtol=0, atol=1e-15)


def test_transfer_interpolates_trilinear_fields():
    """fine vertex = the coarse element's trilinear map at a lattice point; a coarse field interpolated there with the oracle's basis
    equals the transfer applied to it"""
    coarse = _perturbed(2, seed=7)
    fine, t = fa.refine_uniformly_with_transfer(coarse)
    rng = np.random.default_rng(1)
    field = rng.standard_normal((coarse.num_nodes(), 2))
    via_t = t.apply(field)
    pos = t.apply(coarse.vertices)
    assert np.allclose(pos, fine.vertices, rtol=0, atol=1e-14)
    # every child's vertices: the parent's lattice points (-1, 0, 1)^3
    sgn = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], dtype=float)
    for e in range(coarse.num_elements()):
        cn = coarse.connectivity[e].astype(np.int64)
        for ch in range(8):
            cx, cy, cz = ch & 1, (ch >> 1) & 1, (ch >> 2) & 1
            child = fine.connectivity[8 * e + ch].astype(np.int64)
            for a in range(8):
                xi = np.array([cx, cy, cz], dtype=float) + (sgn[a] + 1) / 2 - 1.0
                phi = oracle.element_basis(oracle.HEX8, xi)
                assert np.allclose(phi @ field[cn], via_t[child[a]], rtol=0, atol=1e-13)
                assert np.allclose(phi @ coarse.vertices[cn], fine.vertices[child[a]], rtol=0, atol=1e-14)


def test_refined_box_is_the_generators_box_up_to_a_permutation():
    for n in (1, 2, 3):
        fine = fa.refine_uniformly(fa.procedural.create_unit_box_uniform_hex_mesh_3d(n))
        box = fa.procedural.create_unit_box_uniform_hex_mesh_3d(2 * n)
        assert fine.num_nodes() == box.num_nodes() and fine.num_elements() == box.num_elements()
        key = lambda v: np.round(v * 4 * n).astype(np.int64)
        kf, kb = key(fine.vertices), key(box.vertices)
        lut = {tuple(k): i for i, k in enumerate(kb)}
        perm = np.array([lut[tuple(k)] for k in kf])
        assert len(np.unique(perm)) == len(perm)
        assert np.allclose(fine.vertices, box.vertices[perm], rtol=0, atol=1e-15)
        # the same cells, each with the same node order
        cells_f = sorted(tuple(perm[c]) for c in fine.connectivity.astype(np.int64))
        cells_b = sorted(tuple(c) for c in box.connectivity.astype(np.int64))
        assert cells_f == cells_b


def test_permute_transfer_follows_reorder():
    coarse = _perturbed(2, seed=5)
    fine, t = fa.refine_uniformly_with_transfer(coarse)
    mp = fa.reorder.reorder_mesh_par(fine)
    fine2 = mp.apply(fine)
    cp = fa.reorder.reorder_mesh_par(coarse)
    coarse2 = cp.apply(coarse)
    t2 = fa.permute_transfer(t, mp.vertex_permutation(), cp.vertex_permutation())
    assert np.allclose(t2.apply(coarse2.vertices), fine2.vertices, rtol=0, atol=1e-14)
    rng = np.random.default_rng(2)
    f = rng.standard_normal(coarse.num_nodes())
    assert np.allclose(t2.apply(cp.vertex_permutation().apply_to_slice(f)), mp.vertex_permutation().apply_to_slice(t.apply(f)), rtol=0,
                       atol=1e-14)
