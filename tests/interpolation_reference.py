"""Brute-force numpy restatement of the reference's point location, with no spatial index (test infrastructure).

closest_point of Tri3d2Element, Tri3d3Element and Tet4Element statement for statement (src/element/triangle.rs:440-597,
src/element/tetrahedron.rs:572-672, fenris-geometry/src/primitives/line.rs:115-128, 327-337; try_inverse as nalgebra forms it for 2 x 2 and
3 x 3 matrices), batched over a leading axis, and the selection rule of include/fenris_hip.h applied over ALL elements: the InElement
report with the lowest element index, else the smallest d2 = |x(xi) - p|^2, the lower index on a tie.
"""
import numpy as np

EPS = 4.0 * np.finfo(np.float64).eps
TRI_REF = np.array([[-1.0, -1.0], [1.0, -1.0], [-1.0, 1.0]])
TET_REF = np.array([[-1.0, -1.0, -1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]])
TET_FACES = ((0, 2, 1), (0, 1, 3), (1, 2, 3), (0, 3, 2))   # connectivity.rs:537-540


def tri_basis(xi):
    return np.stack([-0.5 * xi[..., 0] - 0.5 * xi[..., 1], 0.5 * xi[..., 0] + 0.5, 0.5 * xi[..., 1] + 0.5], axis=-1)


def tet_basis(xi):
    return np.stack([-0.5 * xi[..., 0] - 0.5 * xi[..., 1] - 0.5 * xi[..., 2] - 0.5, 0.5 * xi[..., 0] + 0.5, 0.5 * xi[..., 1] + 0.5,
                     0.5 * xi[..., 2] + 0.5], axis=-1)


def map_reference_coords(V, xi):
    """x(xi) of linear simplices V (B, nv, gdim) at xi (B, rdim)"""
    N = tri_basis(xi) if V.shape[1] == 3 else tet_basis(xi)
    return np.einsum("bk,bki->bi", N, V)


def _segment_parameter(a, b, p):
    """LineSegment::closest_point_parametric"""
    dirv = b - a
    d2 = np.sum(dirv * dirv, axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d2 == 0.0, 0.0, np.sum((p - a) * dirv, axis=-1) / np.where(d2 == 0.0, 1.0, d2))
    return np.clip(t, 0.0, 1.0)


def _edges_closest(V, p):
    """closest point on the edges (a, b), (b, c), (c, a): (xi (B, 2), dist2 (B,)); the first edge wins a tie (Iterator::min_by)"""
    B = len(V)
    best_d2 = np.full(B, np.inf)
    best_xi = np.zeros((B, 2))
    for k in range(3):
        x1, x2 = V[:, k], V[:, (k + 1) % 3]
        t = _segment_parameter(x1, x2, p)
        q = x1 + (x2 - x1) * t[:, None]
        d2 = np.sum((p - q) ** 2, axis=-1)
        take = (d2 < best_d2) if k else np.ones(B, dtype=bool)
        ra, rb = TRI_REF[k], TRI_REF[(k + 1) % 3]
        xi = ra[None, :] + (rb - ra)[None, :] * t[:, None]
        best_d2 = np.where(take, d2, best_d2)
        best_xi = np.where(take[:, None], xi, best_xi)
    return best_xi, best_d2


def _likely_in_tri(xi):
    return (xi[:, 0] >= -1.0 - EPS) & (xi[:, 1] >= -1.0 - EPS) & (xi[:, 0] + xi[:, 1] <= EPS)


def _likely_in_tet(xi):
    return (xi[:, 0] >= -1.0 - EPS) & (xi[:, 1] >= -1.0 - EPS) & (xi[:, 2] >= -1.0 - EPS) & (xi[:, 0] + xi[:, 1] + xi[:, 2] <= -1.0 + EPS)


def _inverse2(m):
    """(ok, inverse) of (B, 2, 2): Matrix2::try_inverse"""
    det = m[:, 0, 0] * m[:, 1, 1] - m[:, 1, 0] * m[:, 0, 1]
    ok = det != 0.0
    dd = np.where(ok, det, 1.0)
    inv = np.empty_like(m)
    inv[:, 0, 0] = m[:, 1, 1] / dd
    inv[:, 0, 1] = -m[:, 0, 1] / dd
    inv[:, 1, 0] = -m[:, 1, 0] / dd
    inv[:, 1, 1] = m[:, 0, 0] / dd
    return ok, inv


def _inverse3(m):
    """(ok, inverse) of (B, 3, 3): Matrix3::try_inverse"""
    m11, m12, m13 = m[:, 0, 0], m[:, 0, 1], m[:, 0, 2]
    m21, m22, m23 = m[:, 1, 0], m[:, 1, 1], m[:, 1, 2]
    m31, m32, m33 = m[:, 2, 0], m[:, 2, 1], m[:, 2, 2]
    minor_m12_m23 = m22 * m33 - m32 * m23
    minor_m11_m23 = m21 * m33 - m31 * m23
    minor_m11_m22 = m21 * m32 - m31 * m22
    det = m11 * minor_m12_m23 - m12 * minor_m11_m23 + m13 * minor_m11_m22
    ok = det != 0.0
    dd = np.where(ok, det, 1.0)
    inv = np.empty_like(m)
    inv[:, 0, 0] = minor_m12_m23 / dd
    inv[:, 0, 1] = (m13 * m32 - m33 * m12) / dd
    inv[:, 0, 2] = (m12 * m23 - m22 * m13) / dd
    inv[:, 1, 0] = -minor_m11_m23 / dd
    inv[:, 1, 1] = (m11 * m33 - m31 * m13) / dd
    inv[:, 1, 2] = (m13 * m21 - m23 * m11) / dd
    inv[:, 2, 0] = minor_m11_m22 / dd
    inv[:, 2, 1] = (m12 * m31 - m32 * m11) / dd
    inv[:, 2, 2] = (m11 * m22 - m21 * m12) / dd
    return ok, inv


def tri3d2_closest_point(V, p):
    """Tri3d2Element::closest_point of triangles V (B, 3, 2) and points p (B, 2): (in_element (B,), xi (B, 2))"""
    V, p = np.asarray(V, dtype=np.float64), np.asarray(p, dtype=np.float64)
    a, b, c = V[:, 0], V[:, 1], V[:, 2]
    A = np.stack([0.5 * (b - a), 0.5 * (c - a)], axis=-1)          # X G^T
    p0 = 0.5 * b + 0.5 * c                                         # x(0, 0)
    ok, inv = _inverse2(A)
    xi_interior = np.einsum("bij,bj->bi", inv, p - p0)
    interior = ok & _likely_in_tri(xi_interior)
    xi_edge, dist2_edge = _edges_closest(V, p)
    dist2_interior = np.sum((p - map_reference_coords(V, xi_interior)) ** 2, axis=-1)
    in_element = interior & (dist2_interior < dist2_edge)
    return in_element, np.where(in_element[:, None], xi_interior, xi_edge)


def tri3d3_closest_point(V, p):
    """Tri3d3Element::closest_point (always ClosestPoint) of triangles V (B, 3, 3) and points p (B, 3): xi (B, 2)"""
    a, b, c = V[:, 0], V[:, 1], V[:, 2]
    A = np.stack([0.5 * (b - a), 0.5 * (c - a)], axis=-1)          # (B, 3, 2)
    p0 = 0.5 * b + 0.5 * c
    ATA = np.einsum("bki,bkj->bij", A, A)
    ok, inv = _inverse2(ATA)
    xi_interior = np.einsum("bij,bj->bi", inv, np.einsum("bki,bk->bi", A, p - p0))
    interior = ok & _likely_in_tri(xi_interior)
    xi_edge, dist2_edge = _edges_closest(V, p)
    dist2_interior = np.sum((p - map_reference_coords(V, xi_interior)) ** 2, axis=-1)
    use = interior & (dist2_interior < dist2_edge)
    return np.where(use[:, None], xi_interior, xi_edge)


def tet4_closest_point(V, p):
    """Tet4Element::closest_point of tetrahedra V (B, 4, 3) and points p (B, 3): (in_element (B,), xi (B, 3))"""
    V, p = np.asarray(V, dtype=np.float64), np.asarray(p, dtype=np.float64)
    B = len(V)
    A = np.stack([0.5 * (V[:, k + 1] - V[:, 0]) for k in range(3)], axis=-1)
    p0 = map_reference_coords(V, np.zeros((B, 3)))
    ok, inv = _inverse3(A)
    xi_interior = np.einsum("bij,bj->bi", inv, p - p0)
    interior = ok & _likely_in_tet(xi_interior)
    best_d2 = np.full(B, np.inf)
    best_xi = np.zeros((B, 3))
    for f, face in enumerate(TET_FACES):
        Vf = V[:, face, :]
        xi_f = tri3d3_closest_point(Vf, p)
        d2 = np.sum((map_reference_coords(Vf, xi_f) - p) ** 2, axis=-1)
        take = (d2 < best_d2) if f else np.ones(B, dtype=bool)
        ref_face = np.broadcast_to(TET_REF[list(face)], (B, 3, 3))
        xi = map_reference_coords(ref_face, xi_f)
        best_d2 = np.where(take, d2, best_d2)
        best_xi = np.where(take[:, None], xi, best_xi)
    dist2_interior = np.sum((p - map_reference_coords(V, xi_interior)) ** 2, axis=-1)
    in_element = interior & (dist2_interior < best_d2)
    return in_element, np.where(in_element[:, None], xi_interior, best_xi)


def closest_point(V, p):
    """(in_element, xi, d2) of linear simplices V (B, d + 1, d) and points p (B, d)"""
    in_element, xi = tri3d2_closest_point(V, p) if V.shape[2] == 2 else tet4_closest_point(V, p)
    d2 = np.sum((map_reference_coords(V, xi) - p) ** 2, axis=-1)
    return in_element, xi, d2


def locate_all(vertices, connectivity, points):
    """Every element's report for every point: (in_element (m, E), xi (m, E, d), d2 (m, E)).  connectivity: the vertex nodes first."""
    vertices = np.asarray(vertices, dtype=np.float64)
    d = vertices.shape[1]
    V = vertices[np.asarray(connectivity, dtype=np.int64)[:, : d + 1]]
    points = np.asarray(points, dtype=np.float64).reshape(-1, d)
    m, E = len(points), len(V)
    ins, xis, d2s = np.zeros((m, E), dtype=bool), np.zeros((m, E, d)), np.zeros((m, E))
    for i in range(m):
        ins[i], xis[i], d2s[i] = closest_point(V, np.broadcast_to(points[i], (E, d)))
    return ins, xis, d2s


def select(ins, d2s):
    """the selection rule: per point the lowest InElement, else the smallest d2 (argmin takes the lowest index on a tie)"""
    any_in = ins.any(axis=1)
    return np.where(any_in, np.argmax(ins, axis=1), np.argmin(d2s, axis=1))


def locate(vertices, connectivity, points):
    """(element (m,), xi (m, d), in_element (m,), d2 (m,), runner_up (m,)): the answer of the rule and, for the gap rule of the tests, the
    smallest distance (not squared) of any OTHER element"""
    ins, xis, d2s = locate_all(vertices, connectivity, points)
    m = len(ins)
    e = select(ins, d2s)
    rows = np.arange(m)
    others = np.sqrt(d2s)
    others[rows, e] = np.inf
    return e, xis[rows, e], ins[rows, e], d2s[rows, e], others.min(axis=1) if d2s.shape[1] > 1 else np.full(m, np.inf)
