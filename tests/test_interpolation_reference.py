"""Pins tests/interpolation_reference.py, the numpy restatement that tests/test_interpolation.py compares the device against, to the
reference's own tests: spatially_indexed_tet4_find_closest (tests/integration_tests/interpolation.rs:367-387), the closest-point cases of
tests/unit_tests/element/{triangle,tetrahedron}.rs and tests/unit_tests/spatially_indexed.rs, and the invariants of the answer.  No GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import interpolation_reference as ir  # noqa: E402

import fenris_amd as fa  # noqa: E402
from fenris_amd import quadrature  # noqa: E402

TRI = np.array([[1.0, 0.0], [2.0, 1.0], [-1.0, 2.0]])
BOUNDARY_POINTS = np.array([[-1.0, -1.0], [1.0, -1.0], [-1.0, 1.0], [-1.0, 0.5], [0.5, -1.0], [0.0, 0.0]])


def _diameter(V):
    return max(np.linalg.norm(a - b) for a in V for b in V)


def _one(V, p):
    ins, xi, d2 = ir.closest_point(np.asarray(V, dtype=float)[None], np.asarray(p, dtype=float)[None])
    return bool(ins[0]), xi[0], d2[0]


def test_spatially_indexed_tet4_find_closest():
    mesh = fa.procedural.create_unit_box_uniform_tet_mesh_3d(1)
    _, pts = quadrature.total_order.tetrahedron(0)
    pts = np.asarray(pts).reshape(-1, 3)
    V = mesh.vertices[mesh.connectivity.astype(np.int64)]
    for e in range(mesh.num_elements()):
        for xi_q in pts:
            x_q = ir.map_reference_coords(V[e][None], xi_q[None])[0]
            elem, xi, ins, _, _ = ir.locate(mesh.vertices, mesh.connectivity, x_q[None])
            assert elem[0] == e and ins[0]
            assert np.abs(xi[0] - xi_q).max() <= 1e-12


def test_tri3d2_closest_point_is_a_vertex():
    for p, ref in (([5.0, 2.0], 1), ([2.0, -1.0], 0), ([-3.0, 2.0], 2)):
        ins, xi, _ = _one(TRI, p)
        assert not ins
        assert np.abs(xi - ir.TRI_REF[ref]).max() <= 1e-9 * _diameter(TRI)


def test_tri3d2_closest_point_interior_point():
    xi0 = np.array([-0.5, -0.5])
    x = ir.map_reference_coords(TRI[None], xi0[None])[0]
    ins, xi, _ = _one(TRI, x)
    assert ins and np.abs(xi - xi0).max() <= 1e-9 * _diameter(TRI)


def test_tri3d2_closest_point_degenerate_elements():
    V = np.array([[3.0, 3.0]] * 3)                       # a single point
    _, xi, _ = _one(V, [2.0, 2.0])
    assert np.abs(ir.map_reference_coords(V[None], xi[None])[0] - V[0]).max() <= 1e-12
    V = np.array([[1.0, 1.0], [2.0, 1.0], [0.5, 1.0]])    # a line
    _, xi, _ = _one(V, [1.3, 1.5])
    assert np.abs(ir.map_reference_coords(V[None], xi[None])[0] - [1.3, 1.0]).max() <= 1e-12
    eps = 1e-15                                          # almost a line
    V = np.array([[1.0, 1.0], [3.0, 2.0], [2.0, 1.5 + eps]])
    x = np.array([2.0, 1.5 + eps / 2.0])
    _, xi, _ = _one(V, x)
    assert np.abs(ir.map_reference_coords(V[None], xi[None])[0] - x).max() <= 1e-12


def test_tri3d2_closest_point_boundary_points_and_closest_element_at_interfaces():
    mesh = fa.procedural.create_unit_square_uniform_tri_mesh_2d(10)
    V = mesh.vertices[mesh.connectivity.astype(np.int64)]
    E = len(V)
    for xi0 in BOUNDARY_POINTS:
        X = ir.map_reference_coords(V, np.broadcast_to(xi0, (E, 2)))
        _, xi, _ = ir.closest_point(V, X)                          # tri3d2_closest_point_boundary_points
        assert np.abs(xi - xi0).max() <= 1e-12
        elem, xi_c, _, _, _ = ir.locate(mesh.vertices, mesh.connectivity, X)   # spatially_indexed_closest_element_at_interfaces
        assert np.abs(ir.map_reference_coords(V[elem], xi_c) - X).max() <= 1e-12


def test_tet4_closest_point_failure_case():
    V = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.5, 0.5, 0.5]])
    p = np.array([0.875, 0.375, 0.375])
    ins, xi, d2 = _one(V, p)
    assert not ins and d2 > 0.0
    assert np.any(ir.map_reference_coords(V[None], xi[None])[0] != p)


def test_voronoi_regions_of_a_tetrahedron_and_a_triangle_in_space():
    """the idea of the reference's property tests: a point moved off a face / vertex along the outward direction comes back to it"""
    rng = np.random.default_rng(7)
    V = np.array([[0.1, 0.0, 0.2], [1.3, 0.2, 0.0], [0.2, 1.1, 0.1], [0.3, 0.2, 0.9]])
    for face in ir.TET_FACES:
        a, b, c = V[list(face)]
        n = np.cross(b - a, c - a)
        n /= np.linalg.norm(n)
        w = rng.dirichlet(np.ones(3))
        x0 = w @ V[list(face)]
        ins, xi, d2 = _one(V, x0 + 0.3 * n)
        assert not ins
        assert np.abs(ir.map_reference_coords(V[None], xi[None])[0] - x0).max() <= 1e-12 and abs(d2 - 0.09) <= 1e-12
        xi2 = ir.tri3d3_closest_point(V[list(face)][None], (x0 + 0.3 * n)[None])[0]
        assert np.abs(ir.map_reference_coords(V[list(face)][None], xi2[None])[0] - x0).max() <= 1e-12
    centre = V.mean(axis=0)
    for k in range(4):
        ins, xi, _ = _one(V, V[k] + 0.5 * (V[k] - centre))
        assert not ins and np.abs(xi - ir.TET_REF[k]).max() <= 1e-12
    ins, xi, d2 = _one(V, centre)
    assert ins and d2 <= 1e-28 and np.abs(xi - (-0.5)).max() <= 1e-12


def test_invariants_of_the_answer():
    rng = np.random.default_rng(11)
    for mesh in (fa.procedural.create_unit_square_uniform_tri_mesh_2d(3), fa.procedural.create_unit_box_uniform_tet_mesh_3d(2)):
        d = mesh.vertices.shape[1]
        pts = rng.uniform(-0.5, 1.5, (60, d))
        ins, xis, d2s = ir.locate_all(mesh.vertices, mesh.connectivity, pts)
        elem, xi, in_e, d2, runner = ir.locate(mesh.vertices, mesh.connectivity, pts)
        tol = 4.0 * np.finfo(float).eps
        assert np.all(xi >= -1.0 - 1e-12) and np.all(xi.sum(axis=1) <= (2.0 - d) + 1e-12)   # in the reference simplex
        inside = np.all((pts >= 0.0) & (pts <= 1.0), axis=1)
        assert np.all(in_e[inside & (runner > 1e-9)])                                        # a point well inside one element is in it
        for i in range(len(pts)):
            if in_e[i]:
                assert elem[i] == np.flatnonzero(ins[i])[0] and np.all(xi[i] >= -1.0 - tol)
            else:
                assert not ins[i].any() and d2[i] == d2s[i].min() and elem[i] == np.flatnonzero(d2s[i] == d2[i])[0]
        assert np.all(np.sqrt(d2) <= runner)                                                  # no other element is closer
