"""Point location and interpolation at arbitrary points on the device (fh_locate_points, fh_interpolator_*, fenris_amd.interpolate)
against the in-element evaluation (the reference's integration tests, tests/integration_tests/interpolation.rs) and against the numpy
brute force of tests/interpolation_reference.py.  DESIGN.md section 3.8."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import interpolation_reference as ir  # noqa: E402

import fenris_amd as fa  # noqa: E402
from fenris_amd import _ffi, quadrature  # noqa: E402
from fenris_amd._ffi import FH_BAD_ARGUMENT, FH_INVALID_STATE, FH_UNSUPPORTED  # noqa: E402
from fenris_amd.interpolate import FixedInterpolator, SpatiallyIndexed, ValuesOrGradients  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("fh_point_index_build", "fh_locate_points", "fh_locate_points_dev", "fh_interpolator_create", "fh_interpolator_create_dev",
         "fh_interpolator_from_compressed", "fh_interpolator_destroy", "fh_interpolator_last_error", "fh_interpolator_sizes",
         "fh_interpolator_data", "fh_interpolator_apply", "fh_interpolator_apply_dev", "fh_interpolator_apply_gradients",
         "fh_interpolator_apply_gradients_dev")
NONE = np.uint64(2**64 - 1)


# ---------------------------------------------------------------------------------------------------------------- no GPU
def test_abi_names():
    lib = _ffi.lib()
    for name in NAMES:
        assert name in _ffi.exported_symbols() and getattr(lib, name) is not None
    header = open(os.path.join(ROOT, "include", "fenris_hip.h")).read()
    assert all(name + "(" in header for name in NAMES)
    for name in ("SpatiallyIndexed", "FixedInterpolator", "ValuesOrGradients"):
        assert hasattr(fa, name)
    assert FixedInterpolator.from_space_and_points_par.__func__ is FixedInterpolator.from_space_and_points.__func__
    assert ValuesOrGradients.Both.compute_values() and ValuesOrGradients.Both.compute_gradients()
    assert not ValuesOrGradients.OnlyValues.compute_gradients() and not ValuesOrGradients.OnlyGradients.compute_values()


def _code(fn, *args, **kw):
    with pytest.raises(fa.FenrisError) as err:
        fn(*args, **kw)
    return err.value.code


def test_from_compressed_values_argument_validation():
    """the assertions of FixedInterpolator::from_compressed_values (fixed_interpolator.rs:207-230), raised before any device is touched"""
    f = FixedInterpolator.from_compressed_values
    assert _code(f, [1.0, 2.0], None, [0, 1], [0, 3]) == FH_BAD_ARGUMENT                # an offset beyond the indices
    assert _code(f, [1.0], None, [0, 1], [0, 2]) == FH_BAD_ARGUMENT                     # values and indices differ in number
    assert _code(f, None, [1.0, 2.0, 3.0], [0, 1], [0, 2]) == FH_BAD_ARGUMENT           # gradients no multiple of the indices
    assert _code(f, None, [1.0], [], [0]) == FH_BAD_ARGUMENT                            # gradients without indices
    assert _code(f, [1.0, 2.0], None, [0, 1], [0, 2, 1]) == FH_BAD_ARGUMENT             # decreasing offsets
    assert _code(f, None, np.ones(8), [0, 1], [0, 2]) == FH_BAD_ARGUMENT                # four values per gradient


# ------------------------------------------------------------------------------------------------------------------- fields
def u_scalar_2d(p):
    x, y = p[:, 0], p[:, 1]
    return ((np.cos(x) + np.sin(y)) * x**2)[:, None]


def u_vector_2d(p):
    x, y = p[:, 0], p[:, 1]
    return np.stack([(np.cos(x) + np.sin(y)) * x**2, np.log(x**2 + 0.5) * np.log(y**2 + 0.25) + x * y + 3.0], axis=1)


def u_scalar_3d(p):
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return ((np.cos(x) + np.sin(y) + np.exp(z)) * x**2 * z + 3.0)[:, None]


def u_vector_3d(p):
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([(np.cos(x) + np.sin(y) + np.exp(z)) * x**2 * z + 3.0,
                     np.log(x**2 * z + 0.5) * np.log(z**3 + y**2 + 0.25) + x * y + 4.0,
                     (np.exp(z) * np.exp(x) + y**2) ** 2 + z**3 * x + 5.0], axis=1)


TRI_INTERFACE = np.array([[-1.0, -1.0], [1.0, -1.0], [-1.0, 1.0], [-1.0, 0.5], [0.5, -1.0], [0.0, 0.0]])
TET_INTERFACE = np.array([[-1.0, -1.0, -1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0], [-1 / 3, -1 / 3, -1 / 3]])


def _vertex_cells(mesh):
    d = mesh.vertices.shape[1]
    return mesh.vertices[mesh.connectivity.astype(np.int64)[:, : d + 1]]


def _points_of_elements(mesh, ref_points):
    """(x (E q, d), source element (E q,)): the reference points of every element in physical space"""
    V = _vertex_cells(mesh)
    E, q = len(V), len(ref_points)
    Vr = np.repeat(V, q, axis=0)
    xi = np.tile(ref_points, (E, 1))
    return ir.map_reference_coords(Vr, xi), np.repeat(np.arange(E), q), xi


def _linear_expected(mesh, u, sdim, src, xi):
    """value (m, s) and gradient (m, s, d) of the linear interpolant inside the source elements"""
    conn = mesh.connectivity.astype(np.int64)
    V = _vertex_cells(mesh)[src]
    d = V.shape[2]
    N = ir.tri_basis(xi) if d == 2 else ir.tet_basis(xi)
    un = u.reshape(-1, sdim)[conn[src]]                                   # (m, d + 1, s)
    val = np.einsum("mk,mks->ms", N, un)
    # u(x) = u_0 + (x - v_0) . g with (v_k - v_0) . g = u_k - u_0
    A = V[:, 1:] - V[:, :1]
    g = np.linalg.solve(A, un[:, 1:] - un[:, :1])                         # (m, d, s)
    return val, np.transpose(g, (0, 2, 1))


@pytest.fixture(scope="module")
def engine():
    eng = fa.Engine(0)
    yield eng
    eng.close()


# ---------------------------------------------------------------------------------- 1. the reference's integration tests
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["tri", "tet"])
def test_spatially_indexed_interpolation(engine, case):
    if case == "tri":
        mesh = fa.procedural.create_unit_square_uniform_tri_mesh_2d(10)
        interior, interface, fields = np.asarray(quadrature.total_order.triangle(4)[1]).reshape(-1, 2), TRI_INTERFACE, (u_scalar_2d, u_vector_2d)
    else:
        mesh = fa.procedural.create_unit_box_uniform_tet_mesh_3d(1)
        interior, interface, fields = np.asarray(quadrature.total_order.tetrahedron(2)[1]).reshape(-1, 3), TET_INTERFACE, (u_scalar_3d, u_vector_3d)
    indexed = SpatiallyIndexed.from_space(mesh, engine)
    x, src, xi = _points_of_elements(mesh, interior)
    elem, xi_dev = indexed.find_closest_element_and_reference_coords(x)
    assert np.array_equal(elem.astype(np.int64), src)
    assert np.abs(xi_dev - xi).max() <= 1e-12
    xb, srcb, xib = _points_of_elements(mesh, interface)
    for field in fields:
        un = field(mesh.vertices)
        s = un.shape[1]
        u = un.ravel()
        val, grad = _linear_expected(mesh, u, s, src, xi)
        got = indexed.interpolate_at_points(x, u, s)
        got_grad = indexed.interpolate_gradient_at_points(x, u, s)
        print(case, s, "interior value", np.abs(got - val).max(), "gradient", np.abs(got_grad - grad).max())
        assert np.abs(got - val).max() <= 1e-12
        assert np.abs(got_grad - grad).max() <= 1e-12
        valb, _ = _linear_expected(mesh, u, s, srcb, xib)
        gotb = indexed.interpolate_at_points(xb, u, s)
        print(case, s, "interface value", np.abs(gotb - valb).max())
        assert np.abs(gotb - valb).max() <= 1e-12


# ------------------------------------------------------------------------------------------------------------- 2. kinds
def _poly(d, degree):
    """a polynomial of the degree in d variables and its gradient"""
    if d == 2:
        if degree == 2:
            return (lambda p: 1.0 + p[:, 0] - 2.0 * p[:, 1] + 1.5 * p[:, 0] ** 2 - p[:, 0] * p[:, 1] + 0.5 * p[:, 1] ** 2,
                    lambda p: np.stack([1.0 + 3.0 * p[:, 0] - p[:, 1], -2.0 - p[:, 0] + p[:, 1]], axis=1))
    x, y, z = (lambda p: p[:, 0]), (lambda p: p[:, 1]), (lambda p: p[:, 2])
    if degree == 2:
        return (lambda p: 1.0 + x(p) - 2.0 * y(p) + 0.5 * z(p) + 1.5 * x(p) ** 2 - x(p) * y(p) + 0.5 * y(p) * z(p) + z(p) ** 2,
                lambda p: np.stack([1.0 + 3.0 * x(p) - y(p), -2.0 - x(p) + 0.5 * z(p), 0.5 + 0.5 * y(p) + 2.0 * z(p)], axis=1))
    return (lambda p: 2.0 - x(p) + y(p) * z(p) + x(p) ** 3 - 2.0 * x(p) * y(p) * z(p) + y(p) ** 2 * z(p) + 0.5 * z(p) ** 3,
            lambda p: np.stack([-1.0 + 3.0 * x(p) ** 2 - 2.0 * y(p) * z(p), z(p) - 2.0 * x(p) * z(p) + 2.0 * y(p) * z(p),
                                y(p) - 2.0 * x(p) * y(p) + y(p) ** 2 + 1.5 * z(p) ** 2], axis=1))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["tri6", "tet10", "tet20"])
def test_kinds_reproduce_polynomials_of_their_degree(engine, kind):
    """Tolerances: values 1e-12 max|u|; gradients 1e-11 max|u| / L with L = 1 the edge of the unit domain (the stricter reading of
    'the mesh size': the cell size would allow ten times as much on the triangle mesh)."""
    if kind == "tri6":
        lin = fa.procedural.create_unit_square_uniform_tri_mesh_2d(10)
        mesh, degree, interior = fa.tri6_mesh_from_tri3(lin), 2, np.asarray(quadrature.total_order.triangle(4)[1]).reshape(-1, 2)
    else:
        lin = fa.procedural.create_unit_box_uniform_tet_mesh_3d(1)
        mesh, degree = (fa.tet10_mesh_from_tet4(lin), 2) if kind == "tet10" else (fa.tet20_mesh_from_tet4(lin), 3)
        interior = np.asarray(quadrature.total_order.tetrahedron(2)[1]).reshape(-1, 3)
    d = mesh.vertices.shape[1]
    f, df = _poly(d, degree)
    u = f(mesh.vertices)
    mag = np.abs(u).max()
    indexed = SpatiallyIndexed.from_space(mesh, engine)
    x, src, xi = _points_of_elements(mesh, interior)
    elem, xi_dev = indexed.find_closest_element_and_reference_coords(x)
    assert np.array_equal(elem.astype(np.int64), src) and np.abs(xi_dev - xi).max() <= 1e-12
    fixed = FixedInterpolator.from_space_and_points(indexed, x, ValuesOrGradients.Both)
    off, idx, _, _ = fixed.data()
    n = mesh.connectivity.shape[1]
    assert np.array_equal(off, n * np.arange(len(x) + 1)) and np.array_equal(idx.reshape(-1, n), mesh.connectivity[src])
    val = fixed.interpolate(u, 1)[:, 0]
    grad = fixed.interpolate_gradients(u, 1)[:, 0, :]
    print(kind, "value", np.abs(val - f(x)).max() / mag, "gradient", np.abs(grad - df(x)).max() / mag)
    assert np.abs(val - f(x)).max() <= 1e-12 * mag
    assert np.abs(grad - df(x)).max() <= 1e-11 * mag / 1.0
    # two components: the second is the first scaled
    u2 = np.stack([u, -2.0 * u], axis=1).ravel()
    assert np.array_equal(fixed.interpolate(u2, 2)[:, 0], val) and np.array_equal(fixed.interpolate(u2, 2)[:, 1], -2.0 * val)


# ------------------------------------------------------------------------------------------- 3. against the brute force
def _extrapolation_base_mesh(engine):
    s = 0.0
    v = np.array([[-s, -s], [1.0, -s], [2.0, -s], [3.0 + s, -s], [-s, 1.0], [1.0 + s, 1.0 + s], [2.0 - s, 1.0 + s], [3.0 + s, 1.0 + s],
                  [0.0 - s, 2.0 - s], [1.0 + s, 2.0 - s], [2.0 - s, 2.0 - s], [3.0 + s, 2.0 - s], [0.0 - s, 3.0 + s], [1.0, 3.0 + s],
                  [2.0, 3.0 + s], [3.0 + s, 3.0 + s]])
    c = np.array([[0, 1, 4], [1, 5, 4], [1, 2, 6], [1, 5, 6], [2, 3, 6], [3, 7, 6], [6, 7, 11], [6, 11, 10], [10, 11, 14], [11, 15, 14],
                  [10, 14, 9], [9, 14, 13], [12, 9, 13], [8, 9, 12], [4, 9, 8], [4, 5, 9]], dtype=np.uint64)
    return fa.refine_uniformly_repeat(fa.Mesh(v, c, fa.TRI3), 2, engine)


def _boundary_faces(mesh):
    """(faces (F, d) vertex indices, outward unit normals (F, d)) of the faces that belong to one cell"""
    d = mesh.vertices.shape[1]
    conn = mesh.connectivity.astype(np.int64)[:, : d + 1]
    seen = {}
    for e, cell in enumerate(conn):
        for k in range(d + 1):
            face = tuple(np.delete(cell, k))
            seen.setdefault(tuple(sorted(face)), []).append((face, cell[k]))
    faces, normals = [], []
    for entries in seen.values():
        if len(entries) != 1:
            continue
        face, opposite = entries[0]
        P = mesh.vertices[list(face)]
        nrm = np.array([P[1, 1] - P[0, 1], P[0, 0] - P[1, 0]]) if d == 2 else np.cross(P[1] - P[0], P[2] - P[0])
        nrm = nrm / np.linalg.norm(nrm)
        if np.dot(nrm, mesh.vertices[opposite] - P[0]) > 0:
            nrm = -nrm
        faces.append(face)
        normals.append(nrm)
    return np.array(faces), np.array(normals)


def point_sets(mesh, seed, hole=None):
    """name -> points.  'vertices' and 'faces_edges' lie exactly on interfaces; the other sets are generic."""
    rng = np.random.default_rng(seed)
    d = mesh.vertices.shape[1]
    V = _vertex_cells(mesh)
    E = len(V)
    lo, hi = mesh.vertices.min(axis=0), mesh.vertices.max(axis=0)
    diam = np.linalg.norm(hi - lo)
    sets = {}
    w = rng.dirichlet(np.ones(d + 1), 135)
    sets["inside"] = np.einsum("mk,mki->mi", w, V[rng.integers(0, E, 135)])
    valence = np.bincount(mesh.connectivity.astype(np.int64)[:, : d + 1].ravel(), minlength=len(mesh.vertices))
    sets["vertices"] = mesh.vertices[np.argsort(-valence, kind="stable")[:40]].copy()
    w = rng.dirichlet(np.ones(d + 1), 50)
    w[:25, 0] = 0.0                       # on the face opposite vertex 0
    w[25:, :2] = 0.0 if d == 2 else w[25:, :2]
    if d == 3:
        w[25:, 0] = 0.0                   # on the edge (2, 3)
        w[25:, 1] = 0.0
    w /= w.sum(axis=1, keepdims=True)
    sets["faces_edges"] = np.einsum("mk,mki->mi", w, V[rng.integers(0, E, 50)])
    faces, normals = _boundary_faces(mesh)
    if hole is not None:                  # the faces of the outer boundary only
        mid = mesh.vertices[faces].mean(axis=1)
        outer = ~np.all((mid >= hole[0] - 1e-9) & (mid <= hole[1] + 1e-9), axis=1)
        faces_out, normals_out = faces[outer], normals[outer]
    else:
        faces_out, normals_out = faces, normals
    pick = rng.integers(0, len(faces), 40)
    w = rng.dirichlet(4.0 * np.ones(d), 40)
    sets["just_outside"] = np.einsum("mk,mki->mi", w, mesh.vertices[faces[pick]]) + 1e-6 * diam * normals[pick]
    far = []
    for a in range(d):
        for sign in (1.0, -1.0):          # ten diameters along each of the 2 d directions, over the faces that face it
            align = normals_out[:, a] * sign
            best = np.argsort(-align, kind="stable")[:6]
            w = rng.dirichlet(4.0 * np.ones(d), len(best))
            far.append(np.einsum("mk,mki->mi", w, mesh.vertices[faces_out[best]]) + 10.0 * diam * normals_out[best])
    sets["far_outside"] = np.concatenate(far)
    if hole is not None:
        sets["hole"] = rng.uniform(hole[0] + 0.02, hole[1] - 0.02, (35, d))
    return sets, diam


def _brute_force_meshes(engine):
    return {"sphere_tet4_593": (fa.io.load_msh_from_file(os.path.join(GOLDEN, "msh", "sphere_tet4_593.msh"), fa.TET4), None),
            "box_tet4_res3": (fa.procedural.create_unit_box_uniform_tet_mesh_3d(3), None),
            "extrapolation_tri3": (_extrapolation_base_mesh(engine), (np.array([1.0, 1.0]), np.array([2.0, 2.0])))}


SEED = 20240917
_brute_cache = {}


def _brute(engine, name):
    """mesh, sets, the reference's answers and the device's, computed once per mesh"""
    if name not in _brute_cache:
        mesh, hole = _brute_force_meshes(engine)[name]
        sets, diam = point_sets(mesh, SEED, hole)
        names = list(sets)
        pts = np.concatenate([sets[k] for k in names])
        label = np.concatenate([np.full(len(sets[k]), i) for i, k in enumerate(names)])
        ref = ir.locate(mesh.vertices, mesh.connectivity, pts)
        indexed = SpatiallyIndexed.from_space(mesh, engine)
        dev = indexed.locate(pts)
        u = (u_scalar_2d if mesh.vertices.shape[1] == 2 else u_scalar_3d)(mesh.vertices).ravel()
        val = indexed.interpolate_at_points(pts, u, 1)[:, 0]
        _brute_cache[name] = (mesh, names, pts, label, diam, ref, dev, u, val)
    return _brute_cache[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sphere_tet4_593", "box_tet4_res3", "extrapolation_tri3"])
def test_against_brute_force(engine, name):
    mesh, names, pts, label, diam, ref, dev, u, val = _brute(engine, name)
    assert len(pts) % 64 != 0 and 290 <= len(pts) <= 330          # about 300
    e_ref, xi_ref, in_ref, d2_ref, runner = ref
    e_dev, xi_dev, in_dev = dev
    assert np.all(e_dev != NONE)
    e_dev = e_dev.astype(np.int64)
    V = _vertex_cells(mesh)
    conn = mesh.connectivity.astype(np.int64)
    dist_dev = np.linalg.norm(ir.map_reference_coords(V[e_dev], xi_dev) - pts, axis=1)
    print(name, "distance", np.abs(dist_dev - np.sqrt(d2_ref)).max() / diam)
    assert np.abs(dist_dev - np.sqrt(d2_ref)).max() <= 1e-12 * diam                 # every point
    N = ir.tri_basis(xi_ref) if V.shape[2] == 2 else ir.tet_basis(xi_ref)
    val_ref = np.einsum("mk,mk->m", N, u[conn[e_ref]])
    umax = np.abs(u).max()
    print(name, "value", np.abs(val - val_ref).max() / umax)
    assert np.abs(val - val_ref).max() <= 1e-12 * umax                               # every point: the interpolant is continuous
    clear = runner - np.sqrt(d2_ref) > 1e-9 * diam
    assert np.array_equal(e_dev[clear], e_ref[clear]) and np.array_equal(in_dev[clear], in_ref[clear])
    assert np.abs(xi_dev[clear] - xi_ref[clear]).max() <= 1e-9
    for i, k in enumerate(names):
        left_out = np.count_nonzero(~clear[label == i])
        print(name, k, "points", np.count_nonzero(label == i), "left out by the gap rule", left_out)
        if k not in ("vertices", "faces_edges"):                                     # (those lie on interfaces: distance and value only)
            assert left_out <= 0.1 * np.count_nonzero(label == i)
    xi_sum_max = 2.0 - V.shape[2]
    assert np.all(xi_dev >= -1.0 - 1e-12) and np.all(xi_dev.sum(axis=1) <= xi_sum_max + 1e-12)


def test_generated_point_sets_stay_within_the_gap_cap_on_the_host():
    """the reference alone, no GPU: the generic sets of the two meshes that need no engine leave out at most 10 % by the gap rule"""
    for mesh in (fa.io.load_msh_from_file(os.path.join(GOLDEN, "msh", "sphere_tet4_593.msh"), fa.TET4),
                 fa.procedural.create_unit_box_uniform_tet_mesh_3d(3)):
        sets, diam = point_sets(mesh, SEED)
        assert sum(len(p) for p in sets.values()) % 64 != 0
        for k, pts in sets.items():
            if k in ("vertices", "faces_edges"):
                continue
            _, _, _, d2, runner = ir.locate(mesh.vertices, mesh.connectivity, pts)
            assert np.count_nonzero(runner - np.sqrt(d2) <= 1e-9 * diam) <= 0.1 * len(pts), k


# ------------------------------------------------------------------------------------------------- 4. degenerate input
@pytest.mark.gpu
def test_degenerate_elements(engine):
    box = fa.procedural.create_unit_box_uniform_tet_mesh_3d(1)
    flat = np.array([[i for i, v in enumerate(box.vertices) if v[2] == 0.0][:4]], dtype=np.uint64)   # four vertices of the bottom face
    assert abs(np.linalg.det(box.vertices[flat[0, 1:].astype(int)] - box.vertices[int(flat[0, 0])])) == 0.0
    mesh = fa.Mesh(box.vertices, np.concatenate([flat, box.connectivity]), fa.TET4)   # the element without volume comes first
    indexed = SpatiallyIndexed.from_space(mesh, engine)
    x, src, xi = _points_of_elements(box, np.asarray(quadrature.total_order.tetrahedron(2)[1]).reshape(-1, 3))
    elem, xi_dev, ins = indexed.locate(x)
    assert np.array_equal(elem.astype(np.int64), src + 1) and np.all(ins) and np.abs(xi_dev - xi).max() <= 1e-12
    below = np.array([[0.3, 0.4, -0.3], [0.7, 0.2, -0.05], [0.5, 0.5, -1.0]])
    elem, xi_dev, ins = indexed.locate(below)
    ref = ir.locate(mesh.vertices, mesh.connectivity, below)
    V = _vertex_cells(mesh)
    assert np.all(np.isfinite(xi_dev)) and np.all(xi_dev >= -1.0 - 1e-12) and np.all(xi_dev.sum(axis=1) <= -1.0 + 1e-12) and not ins.any()
    assert np.abs(np.linalg.norm(ir.map_reference_coords(V[elem.astype(np.int64)], xi_dev) - below, axis=1) - np.sqrt(ref[3])).max() <= 1e-12
    # a sliver beside a triangle mesh
    sq = fa.procedural.create_unit_square_uniform_tri_mesh_2d(2)
    nv = len(sq.vertices)
    verts = np.concatenate([sq.vertices, [[1.2, 0.0], [2.2, 0.0], [1.7, 1e-13]]])
    mesh = fa.Mesh(verts, np.concatenate([sq.connectivity, np.array([[nv, nv + 1, nv + 2]], dtype=np.uint64)]), fa.TRI3)
    indexed = SpatiallyIndexed.from_space(mesh, engine)
    x, src, xi = _points_of_elements(sq, np.asarray(quadrature.total_order.triangle(4)[1]).reshape(-1, 2))
    elem, xi_dev, ins = indexed.locate(x)
    assert np.array_equal(elem.astype(np.int64), src) and np.all(ins) and np.abs(xi_dev - xi).max() <= 1e-12
    near = np.array([[1.7, 0.3], [2.0, -0.2], [2.5, 0.0]])
    elem, xi_dev, ins = indexed.locate(near)
    assert np.all(elem == len(sq.connectivity)) and np.all(np.isfinite(xi_dev))
    assert np.all(xi_dev >= -1.0 - 1e-12) and np.all(xi_dev.sum(axis=1) <= 1e-12)
    ref = ir.locate(mesh.vertices, mesh.connectivity, near)
    V = _vertex_cells(mesh)
    assert np.abs(np.linalg.norm(ir.map_reference_coords(V[elem.astype(np.int64)], xi_dev) - near, axis=1) - np.sqrt(ref[3])).max() <= 1e-12


# ------------------------------------------------------------------------------------------------- 5. FixedInterpolator
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["tri", "tet"])
def test_fixed_interpolator_matches_on_demand(engine, case):
    mesh = fa.procedural.create_unit_square_uniform_tri_mesh_2d(1) if case == "tri" else fa.procedural.create_unit_box_uniform_tet_mesh_3d(2)
    d, n = mesh.vertices.shape[1], mesh.connectivity.shape[1]
    rng = np.random.default_rng(5)
    indexed = SpatiallyIndexed.from_space(mesh, engine)
    u = rng.uniform(-1.0, 1.0, 3 * mesh.num_nodes())
    for m in (0, 1, 7, 20):
        pts = rng.uniform(0.0, 1.0, (m, d))
        for what in (ValuesOrGradients.Both, ValuesOrGradients.OnlyValues, ValuesOrGradients.OnlyGradients):
            fixed = FixedInterpolator.from_space_and_points(indexed, pts, what)
            off, idx, val, grad = fixed.data()
            assert np.array_equal(off, n * np.arange(m + 1))
            elem, _ = indexed.find_closest_element_and_reference_coords(pts)
            assert np.array_equal(idx.reshape(m, n), mesh.connectivity[elem.astype(np.int64)].reshape(m, n))
            assert (val is not None) == what.compute_values() and (grad is not None) == what.compute_gradients()
            if what.compute_values():
                got = fixed.interpolate(u, 3)
                assert got.shape == (m, 3) and np.array_equal(got, indexed.interpolate_at_points(pts, u, 3))           # bit-equal
                assert np.array_equal(fixed.to_transfer(mesh.num_nodes()).apply(u.reshape(-1, 3)).reshape(m, 3), got) or \
                    np.abs(fixed.to_transfer(mesh.num_nodes()).apply(u.reshape(-1, 3)).reshape(m, 3) - got).max() <= 1e-15
            else:
                assert _code(fixed.interpolate, u, 3) == FH_INVALID_STATE
            if what.compute_gradients():
                got = fixed.interpolate_gradients(u, 3)
                assert got.shape == (m, 3, d)
                assert np.abs(got - indexed.interpolate_gradient_at_points(pts, u, 3)).max(initial=0.0) <= 1e-9
            else:
                assert _code(fixed.interpolate_gradients, u, 3) == FH_INVALID_STATE
            # round trip through the compressed arrays: the same bits
            again = FixedInterpolator.from_compressed_values(val, grad, idx, off, geometry_dim=d, engine=engine)
            if what.compute_values():
                assert np.array_equal(again.interpolate(u, 3), fixed.interpolate(u, 3))
            if what.compute_gradients():
                assert np.array_equal(again.interpolate_gradients(u, 3), fixed.interpolate_gradients(u, 3))
            if m:
                assert _code(fixed.interpolate if what.compute_values() else fixed.interpolate_gradients, u[:-1], 3) == FH_BAD_ARGUMENT


@pytest.mark.gpu
def test_ragged_offsets_and_sdim(engine):
    off, idx = [0, 2, 2, 5], [3, 1, 0, 2, 4]
    val = np.array([0.25, 0.75, 1.0, -2.0, 0.5])
    grad = np.arange(10.0).reshape(5, 2) - 3.0
    fixed = FixedInterpolator.from_compressed_values(val, grad, idx, off, engine=engine)
    assert fixed.geometry_dim == 2 and fixed.num_points == 3
    rng = np.random.default_rng(3)
    for s in (1, 2, 3):
        u = rng.uniform(-1.0, 1.0, (5, s))
        got, got_grad = fixed.interpolate(u.ravel(), s), fixed.interpolate_gradients(u.ravel(), s)
        for p in range(3):
            acc, accg = np.zeros(s), np.zeros((s, 2))
            for k in range(off[p], off[p + 1]):          # in stored order
                acc = acc + val[k] * u[idx[k]]
                accg = accg + np.outer(u[idx[k]], grad[k])
            assert np.abs(got[p] - acc).max() <= 1e-15 and np.abs(got_grad[p] - accg).max() <= 1e-14
        assert np.all(got[1] == 0.0) and np.all(got_grad[1] == 0.0)    # the empty row
        assert np.array_equal(fixed.to_transfer(5).apply(u), got) or np.abs(fixed.to_transfer(5).apply(u) - got).max() <= 1e-15
        assert _code(fixed.interpolate, u.ravel()[: 5 * s - 1], s) == FH_BAD_ARGUMENT


@pytest.mark.gpu
def test_interpolator_at_the_refined_vertices_is_the_refinement_transfer(engine):
    coarse = fa.procedural.create_unit_box_uniform_tet_mesh_3d(2)
    fine, transfer = fa.refine_uniformly_with_transfer(coarse, engine)
    indexed = SpatiallyIndexed.from_space(coarse, engine)
    fixed = FixedInterpolator.from_space_and_points(indexed, fine.vertices, ValuesOrGradients.OnlyValues)
    a = fixed.to_transfer(coarse.num_nodes()).to_scipy().tocsr()
    b = transfer.to_scipy().tocsr()
    a.sum_duplicates()
    b.sort_indices()
    diff = (a - b).tocoo()
    assert a.shape == b.shape and (np.abs(diff.data).max() if diff.nnz else 0.0) <= 1e-14
    a.data[np.abs(a.data) <= 1e-14] = 0.0                # weights of an element's other nodes at a point on its edge or face
    a.eliminate_zeros()
    b.eliminate_zeros()
    assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)


# -------------------------------------------------------------------------------- 6. lifetime and reproducibility
@pytest.mark.gpu
def test_two_builds_and_two_locates_give_identical_bytes(engine):
    mesh, names, pts, label, diam, ref, dev, u, val = _brute(engine, "sphere_tet4_593")
    for _ in range(2):
        indexed = SpatiallyIndexed.from_space(mesh, engine)          # builds the index again
        for _ in range(2):
            again = indexed.locate(pts)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(again, dev))
        fixed = FixedInterpolator.from_space_and_points(indexed, pts, ValuesOrGradients.Both)
        assert fixed.interpolate(u, 1)[:, 0].tobytes() == val.tobytes()


@pytest.mark.gpu
def test_index_follows_update_vertices_and_hex8_is_unsupported(engine):
    mesh = fa.procedural.create_unit_box_uniform_tet_mesh_3d(2)
    indexed = SpatiallyIndexed.from_space(mesh, engine)
    x, src, xi = _points_of_elements(mesh, np.asarray(quadrature.total_order.tetrahedron(2)[1]).reshape(-1, 3))
    shift = np.array([5.0, -3.0, 2.0])
    moved = 2.0 * mesh.vertices + shift
    engine.update_vertices(moved)                        # drops the index; the next call builds it for the moved mesh
    elem, xi_dev, ins = indexed.locate(2.0 * x + shift)
    assert np.array_equal(elem.astype(np.int64), src) and np.all(ins) and np.abs(xi_dev - xi).max() <= 1e-12
    elem, _, ins = indexed.locate(x[:5])                 # the old places are now outside the mesh
    assert not ins.any()
    assert _code(indexed.locate, np.array([[np.nan, 0.0, 0.0]])) == FH_BAD_ARGUMENT
    hexes = fa.procedural.create_unit_box_uniform_hex_mesh_3d(2)
    engine.set_mesh(hexes)
    assert _code(indexed.locate, x) == FH_UNSUPPORTED
    assert _code(FixedInterpolator.from_space_and_points, indexed, x) == FH_UNSUPPORTED
    assert _code(SpatiallyIndexed.from_space, hexes, engine) == FH_UNSUPPORTED
    assert "Tri3" in engine.last_error()


@pytest.mark.gpu
def test_non_finite_points_on_the_device_entry_point(engine):
    import torch

    mesh = fa.procedural.create_unit_box_uniform_tet_mesh_3d(2)
    indexed = SpatiallyIndexed.from_space(mesh, engine)
    pts = torch.tensor([[0.31, 0.22, 0.13], [float("nan"), 0.1, 0.1], [0.2, float("inf"), 0.1], [0.9, 0.8, 0.7]], dtype=torch.float64, device="cuda")
    elem, xi, ins = indexed.locate(pts)
    torch.cuda.synchronize()
    elem = elem.cpu().numpy().astype(np.uint64)
    assert elem[1] == NONE and elem[2] == NONE and elem[0] != NONE and elem[3] != NONE
    assert np.all(xi.cpu().numpy()[1:3] == 0.0) and list(ins.cpu().numpy()) == [1, 0, 0, 1]
    fixed = FixedInterpolator.from_space_and_points(indexed, pts, ValuesOrGradients.Both)
    u = torch.ones(mesh.num_nodes(), dtype=torch.float64, device="cuda")
    val = fixed.interpolate(u, 1)
    grad = fixed.interpolate_gradients(u, 1)
    torch.cuda.synchronize()
    val = val.cpu().numpy()[:, 0]
    assert val[1] == 0.0 and val[2] == 0.0 and abs(val[0] - 1.0) <= 1e-15 and abs(val[3] - 1.0) <= 1e-15
    assert np.all(grad.cpu().numpy()[1:3] == 0.0)
