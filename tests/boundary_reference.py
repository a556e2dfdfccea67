"""Independent restatements for the boundary search and the surface load (pure Python / numpy, no library code).

1. The search (src/mesh.rs:167-203): a dict of sorted node tuples, a count, sorted() of the keys.
2. The surface integral, written directly: the FACE element's own basis times the cross product of explicit tangents of the face's
   corner geometry, in np.longdouble.  The kernel instead maps the face point into the cell and uses the cell's basis and Jacobian
   (Nanson's formula); a wrong face-to-cell map or reference normal shows as a difference.
"""
import numpy as np

QUAD4, HEX8, TET4, HEX27, TRI3, TET10, QUAD9, TRI6, HEX20, TET20 = range(10)
LD = np.longdouble

# get_face_connectivity (src/connectivity.rs), local node lists per local face
FACES = {
    QUAD4: [[i, (i + 1) % 4] for i in range(4)],                       # :205-212
    TRI3: [[i, (i + 1) % 3] for i in range(3)],                        # :252-259
    TRI6: [[i, i + 3, (i + 1) % 3] for i in range(3)],                 # :340-351
    QUAD9: [[0, 4, 1], [1, 5, 2], [2, 6, 3], [3, 7, 0]],               # :414-423
    TET4: [[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]],                # :532-543
    HEX8: [[3, 2, 1, 0], [0, 1, 5, 4], [1, 2, 6, 5], [2, 3, 7, 6], [4, 7, 3, 0], [5, 6, 7, 4]],   # :616-634
    HEX27: [[0, 3, 2, 1, 9, 13, 11, 8, 20], [0, 1, 5, 4, 8, 12, 16, 10, 21], [1, 2, 6, 5, 11, 14, 18, 12, 23],
            [2, 3, 7, 6, 13, 15, 19, 14, 24], [0, 4, 7, 3, 10, 17, 15, 9, 22], [4, 5, 6, 7, 16, 18, 19, 17, 25]],   # :687-695
    HEX20: [[0, 3, 2, 1, 9, 13, 11, 8], [0, 1, 5, 4, 8, 12, 16, 10], [1, 2, 6, 5, 11, 14, 18, 12],
            [2, 3, 7, 6, 13, 15, 19, 14], [0, 4, 7, 3, 10, 17, 15, 9], [4, 5, 6, 7, 16, 18, 19, 17]],   # :753-760
    TET10: [[0, 2, 1, 6, 5, 4], [0, 1, 3, 4, 9, 7], [1, 2, 3, 5, 8, 9], [0, 3, 2, 7, 8, 6]],   # :930-936
    TET20: [],                                                         # :977-987: no faces
}
FACE_KIND = {QUAD4: "seg2", TRI3: "seg2", TRI6: "seg3", QUAD9: "seg3", TET4: "tri3", TET10: "tri6", HEX8: "quad4", HEX20: "quad8",
             HEX27: "quad9", TET20: None}
CELL_CORNERS = {QUAD4: 4, HEX8: 8, TET4: 4, HEX27: 8, TRI3: 3, TET10: 4, QUAD9: 4, TRI6: 3, HEX20: 8, TET20: 4}


# ---------------------------------------------------------------------------------------------------------------- the search
def find_boundary_faces(kind, connectivity):
    """-> (face_nodes F x nf uint64, cells F uint64, local_faces F uint32) in the reference's order"""
    table = FACES[kind]
    count, first = {}, {}
    for cell, conn in enumerate(np.asarray(connectivity).tolist()):
        for lf, loc in enumerate(table):
            nodes = [conn[a] for a in loc]
            key = tuple(sorted(nodes))
            count[key] = count.get(key, 0) + 1
            first.setdefault(key, (nodes, cell, lf))
    out = [first[k] for k in sorted(count) if count[k] == 1]
    nf = len(table[0]) if table else 1
    fn = np.array([o[0] for o in out], dtype=np.uint64).reshape(len(out), nf)
    return fn, np.array([o[1] for o in out], dtype=np.uint64), np.array([o[2] for o in out], dtype=np.uint32)


def find_boundary_vertices(kind, connectivity):
    return np.unique(find_boundary_faces(kind, connectivity)[0]).astype(np.uint64) if FACES[kind] else np.zeros(0, dtype=np.uint64)


def find_boundary_cells(kind, connectivity):
    return np.unique(find_boundary_faces(kind, connectivity)[1]).astype(np.uint64)


# ------------------------------------------------------------------------------------------------------------ face elements
def _seg2(s):
    return [(1 - s) / 2, (1 + s) / 2]


def _seg3(s):   # nodes at -1, 0, 1 in the order [end, middle, end] of Segment3 (connectivity.rs:343-347, :417)
    return [s * (s - 1) / 2, (1 - s) * (1 + s), s * (s + 1) / 2]


_QS = [(-1, -1), (1, -1), (1, 1), (-1, 1)]


def _quad4(s, t):
    return [(1 + a * s) * (1 + b * t) / 4 for a, b in _QS]


def _quad4_ds(s, t):
    return [a * (1 + b * t) / 4 for a, b in _QS]


def _quad4_dt(s, t):
    return [b * (1 + a * s) / 4 for a, b in _QS]


def _q1(al, x):   # 1D quadratic Lagrange function of the node at al in {-1, 0, 1}
    return x * (x + al) / 2 if al else (1 - x) * (1 + x)


_Q9 = _QS + [(0, -1), (1, 0), (0, 1), (-1, 0), (0, 0)]


def _quad9(s, t):
    return [_q1(a, s) * _q1(b, t) for a, b in _Q9]


def _quad8(s, t):   # serendipity
    out = [(1 + a * s) * (1 + b * t) * (a * s + b * t - 1) / 4 for a, b in _QS]
    for a, b in _Q9[4:8]:
        out.append((1 - s * s) * (1 + b * t) / 2 if a == 0 else (1 - t * t) * (1 + a * s) / 2)
    return out


def _tri3(s, t):   # on (-1,-1), (1,-1), (-1,1)
    return [-(s + t) / 2, (1 + s) / 2, (1 + t) / 2]


def _tri6(s, t):
    l0, l1, l2 = _tri3(s, t)
    return [l0 * (2 * l0 - 1), l1 * (2 * l1 - 1), l2 * (2 * l2 - 1), 4 * l0 * l1, 4 * l1 * l2, 4 * l0 * l2]


FACE_BASIS = {"seg2": _seg2, "seg3": _seg3, "tri3": _tri3, "tri6": _tri6, "quad4": _quad4, "quad8": _quad8, "quad9": _quad9}
FACE_CORNERS = {"seg2": [0, 1], "seg3": [0, 2], "tri3": [0, 1, 2], "tri6": [0, 1, 2], "quad4": [0, 1, 2, 3], "quad8": [0, 1, 2, 3],
                "quad9": [0, 1, 2, 3]}


def face_geometry(fk, xc, pt):
    """x and the area vector a (tangent cross product; 2D: the tangent turned clockwise) at the face point, from the face's CORNER
    vertices xc (the sub-parametric geometry: hexahedron.rs:324-330, tetrahedron.rs:233-240, triangle.rs:258-264)"""
    if fk.startswith("seg"):
        s = pt[0]
        x = xc[0] * (1 - s) / 2 + xc[1] * (1 + s) / 2
        t = (xc[1] - xc[0]) / 2
        return x, np.array([t[1], -t[0]], dtype=LD)
    if fk.startswith("tri"):
        s, t = pt
        e1, e2 = (xc[1] - xc[0]) / 2, (xc[2] - xc[0]) / 2
        return xc[0] + e1 * (s + 1) + e2 * (t + 1), np.cross(e1, e2)
    s, t = pt
    n, ds, dt = _quad4(s, t), _quad4_ds(s, t), _quad4_dt(s, t)
    x = sum(n[i] * xc[i] for i in range(4))
    return x, np.cross(sum(ds[i] * xc[i] for i in range(4)), sum(dt[i] * xc[i] for i in range(4)))


# ----------------------------------------------------------------------------------------------------------------- face rules
def face_rule(fk, n):
    """Gauss rule with n points per direction on the face's reference domain (triangle: collapsed square)"""
    g, w = np.polynomial.legendre.leggauss(n)
    if fk.startswith("seg"):
        return w.copy(), g.reshape(-1, 1).copy()
    if fk.startswith("quad"):
        return np.array([wi * wj for wj in w for wi in w]), np.array([[gi, gj] for gj in g for gi in g])
    ws, ps = [], []
    for v, wv in zip(g, w):
        for u, wu in zip(g, w):
            ps.append([(1 + u) * (1 - v) / 2 - 1, v])
            ws.append(wu * wv * (1 - v) / 2)
    return np.array(ws), np.array(ps)


# ------------------------------------------------------------------------------------------------------------ the surface load
def _item(data, f, q, F, nq, comps):
    d = np.asarray(data, dtype=np.float64).reshape(-1)
    count = d.size // comps
    i = 0 if count == 1 else f if count == F else f * nq + q
    return d[i * comps:(i + 1) * comps].astype(LD)


def face_points(kind, vertices, connectivity, cells, local_faces, points):
    fk = FACE_KIND[kind]
    V = np.asarray(vertices, dtype=LD)
    out = np.zeros((len(cells), len(points), V.shape[1]))
    for f, (cell, lf) in enumerate(zip(cells, local_faces)):
        fn = [int(connectivity[int(cell)][a]) for a in FACES[kind][int(lf)]]
        xc = V[[fn[i] for i in FACE_CORNERS[fk]]]
        for q, pt in enumerate(np.asarray(points, dtype=LD)):
            out[f, q] = face_geometry(fk, xc, pt)[0]
    return out


def surface_load(kind, vertices, connectivity, cells, local_faces, weights, points, sdim, traction=None, pressure=None, data_count=None):
    """out (sdim * N, long double):  traction: += w N t |a|;  pressure: += -w N p a   (per face of the list, per point)"""
    fk = FACE_KIND[kind]
    V = np.asarray(vertices, dtype=LD)
    d = V.shape[1]
    out = np.zeros(sdim * len(V), dtype=LD)
    F, nq = len(cells), len(weights)
    W, P = np.asarray(weights, dtype=LD), np.asarray(points, dtype=LD)
    basis = FACE_BASIS[fk]
    for f, (cell, lf) in enumerate(zip(cells, local_faces)):
        fn = [int(connectivity[int(cell)][a]) for a in FACES[kind][int(lf)]]
        xc = V[[fn[i] for i in FACE_CORNERS[fk]]]
        for q in range(nq):
            _, a = face_geometry(fk, xc, P[q])
            N = basis(*P[q])
            if pressure is not None:
                p = _item(pressure, f, q, F, nq, 1)[0]
                for m, node in enumerate(fn):
                    out[sdim * node:sdim * node + d] += -W[q] * N[m] * p * a
            else:
                t = _item(traction, f, q, F, nq, sdim)
                ds = np.sqrt(np.sum(a * a))
                for m, node in enumerate(fn):
                    out[sdim * node:sdim * node + sdim] += W[q] * N[m] * t * ds
    return out


# ------------------------------------------------------------------------------------------------------- outward normals, areas
def face_area_vectors(kind, vertices, connectivity, cells, local_faces):
    """per face: the integral of the area vector (one-point rule on segments / triangles, 2 x 2 Gauss on quadrilaterals: exact for
    the bilinear face), the face's corner centroid and the cell's corner centroid"""
    fk = FACE_KIND[kind]
    V = np.asarray(vertices, dtype=LD)
    w, p = face_rule(fk, 2)
    A, cf, cc = [], [], []
    for cell, lf in zip(cells, local_faces):
        conn = connectivity[int(cell)]
        fn = [int(conn[a]) for a in FACES[kind][int(lf)]]
        xc = V[[fn[i] for i in FACE_CORNERS[fk]]]
        A.append(sum(LD(wq) * face_geometry(fk, xc, np.asarray(pq, dtype=LD))[1] for wq, pq in zip(w, p)))
        cf.append(xc.mean(axis=0))
        cc.append(V[[int(v) for v in conn[:CELL_CORNERS[kind]]]].mean(axis=0))
    return np.array(A), np.array(cf), np.array(cc)
