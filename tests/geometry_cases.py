"""Stretched, sheared, graded, shifted, scaled and mirrored meshes for test_extreme_geometry.py, and what each of them claims, computed on
the host from the vertices alone (test_geometry_cases.py asserts it).

Base meshes: the smallest that still reach the kernels' internal edges (several tiles with a ragged last one, more than 64 nodes for the
row-owner tables), like test_large_deformation.py.  Every base mesh comes `exact` (the image of the uniform mesh: its Hex8 elements are
parallelepipeds to the classifier) and `jittered` (every vertex moved by up to 0.1 h per axis in the unit box BEFORE the map: no Hex8
element stays affine).  The 2D kinds use the first two axes of every map."""
from types import SimpleNamespace

import numpy as np

import fenris_amd as fa
from fenris_amd import quadrature

KINDS = ("HEX8", "TET4", "QUAD4", "TRI3", "HEX27", "TET10")
VARIANTS = ("exact", "jittered")
SHEAR = np.array([[1.0, 0.98, 0.0], [0.0, 0.2, 0.0], [0.0, 0.97, 0.25]])
SHIFT = np.array([1024.0, -2048.0, 512.0])
LINEAR_MAPS = {"unit": np.eye(3), "plate_1e2": np.diag([1.0, 1.0, 1e-2]), "plate_1e4": np.diag([1.0, 1.0, 1e-4]),
               "needle_1e3": np.diag([1.0, 1e-3, 1e-3]), "shear": SHEAR, "scaled_down": 2.0 ** -20 * np.eye(3),
               "scaled_up": 2.0 ** 20 * np.eye(3), "mirrored": np.diag([-1.0, 1.0, 1.0])}
GEOMETRIES = ("unit", "plate_1e2", "plate_1e4", "needle_1e3", "shear", "graded", "shifted", "scaled_down", "scaled_up", "mirrored")
AFFINE_TOL = 2.0 ** -46            # the default of fh_set_affine_tolerance
HEX_SIGNS = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]])
GEOMETRY_NODES = {"HEX8": 8, "TET4": 4, "QUAD4": 4, "TRI3": 3, "HEX27": 8, "TET10": 4}


def rule_of(kind, gauss=None):
    """(weights, points) of the rule the kind is tested with (gauss: another order of the tensor rules)"""
    if kind in ("HEX8", "HEX27"):
        w, p = quadrature.tensor.hexahedron_gauss(gauss or (3 if kind == "HEX27" else 2))
    elif kind == "QUAD4":
        w, p = quadrature.tensor.quadrilateral_gauss(gauss or 2)
    elif kind == "TRI3":
        w, p = quadrature.total_order.triangle(2)
    else:
        w, p = quadrature.total_order.tetrahedron(2)
    return np.asarray(w), np.asarray(p)


def _base(kind):
    """(linear mesh on a box at the origin, h).  Hex8: h = 1 / 8, so that every coordinate of the base mesh, and of `shifted`, is exactly
    representable and the classifier's sums of the exact variants carry no rounding of their own (with h = 1 / 9 the sums 2 y_j - y_j+1 of
    rounded grid coordinates leave a residue of an ulp of the in-plane coordinates, which a plate's thin edge times 2^-46 is smaller than)"""
    if kind == "HEX8":
        h = 1.0 / 8.0
        return fa.procedural.create_rectangular_uniform_hex_mesh(h, 9, 7, 6, 1), h      # 378 elements
    if kind == "TET4":
        return fa.procedural.create_unit_box_uniform_tet_mesh_3d(4), 0.25                # 768
    if kind == "QUAD4":
        return fa.procedural.create_unit_square_uniform_quad_mesh_2d(20), 0.05
    if kind == "TRI3":
        return fa.procedural.create_unit_square_uniform_tri_mesh_2d(12), 1.0 / 12.0      # 288
    if kind == "HEX27":
        return fa.procedural.create_rectangular_uniform_hex_mesh(0.5, 3, 2, 2, 1), 0.5
    if kind == "TET10":
        return fa.procedural.create_unit_box_uniform_tet_mesh_3d(2), 0.5
    raise ValueError(kind)


def _mapped(v, geometry):
    d = v.shape[1]
    if geometry == "graded":
        return np.expm1(3.0 * v)
    if geometry == "shifted":
        return v + SHIFT[:d]
    return v @ LINEAR_MAPS[geometry][:d, :d].T


def _threshold_vertices(v, h):
    """the plate_1e2 box with a mixed coefficient c_23 (eta zeta) along z in every element: 0.5 x 2^-46 x the shortest linear coefficient
    (c_3 = 1e-2 h / 2) in the element layers with even k, 2 x that in the odd ones.  The field z += j P(k) has the second difference
    P(k + 1) - P(k) in j and k, which is 4 c_23; it does not depend on i, so c_12 = c_31 = c_123 = 0."""
    j, k = np.rint(v[:, 1] / h).astype(int), np.rint(v[:, 2] / h).astype(int)
    out = v @ LINEAR_MAPS["plate_1e2"].T
    c3 = 0.5 * 1e-2 * h
    steps = np.array([4.0 * (0.5 if layer % 2 == 0 else 2.0) * AFFINE_TOL * c3 for layer in range(int(k.max()))])
    P = np.concatenate([[0.0], np.cumsum(steps)])
    out[:, 2] += j * P[k]
    return out


def case(kind, variant, geometry):
    """the mesh of one case with its rule: .mesh (Hex27 / Tet10: elevated from the linear mesh), .linear (the linear mesh), .w, .p, .h (of
    the base mesh), .kind, .variant, .geometry"""
    assert kind in KINDS and variant in VARIANTS and (geometry in GEOMETRIES or (geometry == "threshold" and kind == "HEX8" and variant == "exact"))
    m, h = _base(kind)
    v = np.array(m.vertices, dtype=np.float64)
    if variant == "jittered":
        rng = np.random.default_rng(100 + KINDS.index(kind))         # (one jitter per kind: the geometries map the same mesh)
        v = v + 0.1 * h * rng.uniform(-1.0, 1.0, v.shape)
    v = _threshold_vertices(v, h) if geometry == "threshold" else _mapped(v, geometry)
    linear = fa.Mesh(np.ascontiguousarray(v), m.connectivity, m.elem_kind)
    mesh = fa.hex27_mesh_from_hex8(linear) if kind == "HEX27" else fa.tet10_mesh_from_tet4(linear) if kind == "TET10" else linear
    w, p = rule_of(kind)
    return SimpleNamespace(kind=kind, variant=variant, geometry=geometry, mesh=mesh, linear=linear, w=w, p=p, h=h)


def smooth_u(X, s):
    """a smooth non-zero field on the mesh's bounding box, of the size of the box"""
    lo, hi = X.min(axis=0), X.max(axis=0)
    xi = (X - lo) / (hi - lo)
    L = float((hi - lo).max())
    u = np.zeros((len(X), s))
    for k in range(s):
        a = np.cos(1.0 + np.arange(3) + 2.0 * k)
        u[:, k] = 0.04 * L * (a[0] * np.sin(np.pi * xi[:, 0]) * np.cos(0.5 * np.pi * xi[:, 1]) + a[1] * np.sin(np.pi * xi[:, 1])
                              + a[2] * np.cos(np.pi * xi.sum(axis=1)) + 0.5)
    return u.reshape(-1)


def all_cases():
    out = [(k, v, g) for k in KINDS for v in VARIANTS for g in GEOMETRIES]
    return out + [("HEX8", "exact", "threshold")]


# ---- what a case claims, from the vertices alone
def _element_vertices(c):
    conn = np.asarray(c.linear.connectivity).astype(np.int64)
    return np.asarray(c.linear.vertices, dtype=np.float64)[conn]                         # (E, ng, d)


def centre_jacobians(c):
    """J at the element's centre, (E, d, d): columns = the edge vectors of the reference axes (simplices: the constant J)"""
    X = _element_vertices(c)
    if c.kind in ("HEX8", "HEX27"):
        return np.einsum("eni,nj->eij", X, HEX_SIGNS / 8.0)
    if c.kind == "QUAD4":
        return np.einsum("eni,nj->eij", X, HEX_SIGNS[:4, :2] / 4.0)
    return np.swapaxes(X[:, 1:] - X[:, :1], 1, 2) / 2.0


def properties(c):
    """aspect: the largest ratio of two singular values of J over the elements' centres (the cond of J); det_sign: the signs of det J that
    occur; size_ratio: largest / smallest singular value of J over the whole mesh"""
    J = centre_jacobians(c)
    sv = np.linalg.svd(J, compute_uv=False)
    return SimpleNamespace(aspect=float((sv[:, 0] / sv[:, -1]).max()), det_signs=set(np.sign(np.linalg.det(J)).astype(int).tolist()),
                           size_ratio=float(sv.max() / sv.min()), sv=sv)


def element_gamma(c):
    """gamma_e = 1 + max_a |X_a|_inf / (shortest distance of two vertices of element e): coordinates stored as doubles carry a rounding of
    eps |X|, which enters J, a sum of coordinate differences of size h, at the relative size eps |X| / h whatever the kernel does"""
    X = _element_vertices(c)
    far = np.abs(X).max(axis=(1, 2))
    dist = np.linalg.norm(X[:, :, None, :] - X[:, None, :, :], axis=3)
    n = X.shape[1]
    dist[:, np.arange(n), np.arange(n)] = np.inf
    return 1.0 + far / dist.min(axis=(1, 2))


def gamma_of(c):
    """the factor on the bar: 1 but for `shifted`"""
    return element_gamma(c) if c.geometry == "shifted" else None


def classify_affine_hex8(vertices, connectivity, tol=AFFINE_TOL):
    """k_classify_affine_hex8 restated: the seven coefficient vectors c_k = sum_a sign_k(a) X_a summed node by node in the kernel's order, the
    longest mixed one (c_12, c_23, c_31, c_123) against tol x the shortest linear one (c_1, c_2, c_3); one flag per element"""
    X = np.asarray(vertices, dtype=np.float64)[np.asarray(connectivity).astype(np.int64)]   # (E, 8, 3)
    sx, sy, sz = HEX_SIGNS[:, 0], HEX_SIGNS[:, 1], HEX_SIGNS[:, 2]
    signs = np.stack([sx, sy, sz, sx * sy, sy * sz, sz * sx, sx * sy * sz]).astype(np.float64)   # (7, 8)
    c = np.zeros((len(X), 7, 3))
    for g in range(8):
        c += signs[None, :, g, None] * X[:, None, g, :]
    norm = np.sqrt(c[:, :, 0] * c[:, :, 0] + c[:, :, 1] * c[:, :, 1] + c[:, :, 2] * c[:, :, 2])
    lin_min, dev = norm[:, :3].min(axis=1), norm[:, 3:].max(axis=1)
    return (lin_min > 0.0) & (dev <= tol * lin_min)


def predicted_affine_elements(c):
    """how many Hex8 elements the device will find affine at the default tolerance"""
    assert c.kind == "HEX8"
    return int(classify_affine_hex8(c.linear.vertices, c.linear.connectivity).sum())
