"""numpy restatement of the recovered quantities (fh_recover*), written for tests/test_recovery.py.

Per element and quadrature point: J from the vertex nodes and oracle.element_gradients of the geometry kind, grad u = J^-T sum_n ghat_n
u_n^T, then P and psi from oracle.material_stress_tensor / material_energy_density (the restated fenris-solid materials; Laplace in
closed form) and strain, Cauchy stress and von Mises stress by their definitions.  Element means are measure-weighted sums in point order,
nodal values volume-weighted sums in ascending element order.  Needs the oracle only: no GPU, no fenris_amd.
"""
import numpy as np

QUAD4, HEX8, TET4, HEX27, TRI3, TET10, QUAD9, TRI6, HEX20, TET20 = range(10)
LAPLACE, LINEAR_ELASTIC, NEO_HOOKEAN, STVK = range(4)
KINDS = {"QUAD4": QUAD4, "HEX8": HEX8, "TET4": TET4, "HEX27": HEX27, "TRI3": TRI3, "TET10": TET10, "QUAD9": QUAD9, "TRI6": TRI6,
         "HEX20": HEX20, "TET20": TET20}
OPS = {"LAPLACE": LAPLACE, "LINEAR_ELASTIC": LINEAR_ELASTIC, "NEO_HOOKEAN": NEO_HOOKEAN, "STVK": STVK}
GEOM = {QUAD4: QUAD4, HEX8: HEX8, TET4: TET4, HEX27: HEX8, TRI3: TRI3, TET10: TET4, QUAD9: QUAD4, TRI6: TRI3, HEX20: HEX8, TET20: TET4}
NG = {QUAD4: 4, HEX8: 8, TET4: 4, TRI3: 3}
SOLID = ("strain", "cauchy_stress", "von_mises")
FIELDS = ("grad_u", "strain", "stress_pk1", "cauchy_stress", "von_mises", "energy_density")


def quantities_of(op):
    return [q for q in FIELDS if op != LAPLACE or q not in SOLID]


def linear_mesh(oracle, geom, perturb=0.1, seed=7):
    """the smallest meshes with an interior vertex: 2x2x2 hexahedra, the tetrahedra of tet_mesh(.., 1), 3x3 quadrilaterals and their
    triangles; interior vertices moved by a seeded `perturb` of a cell so that J differs from point to point"""
    if geom == HEX8:
        v, c = oracle.hex_mesh(1.0, 1, 1, 1, 2)
        h = 0.5
    elif geom == TET4:
        v, c = oracle.tet_mesh(1.0, 1, 1, 1, 1)
        h = 1.0
    else:
        v, c = oracle.unit_square_quad_mesh(3)
        h = 1.0 / 3.0
        if geom == TRI3:
            c = np.ascontiguousarray(np.stack([c[:, [0, 1, 2]], c[:, [0, 2, 3]]], axis=1).reshape(-1, 3))
    lo, hi = v.min(axis=0), v.max(axis=0)
    interior = np.all((v > lo + 1e-9) & (v < hi - 1e-9), axis=1)
    assert interior.any()
    rng = np.random.default_rng(seed)
    v = v + perturb * h * rng.uniform(-1.0, 1.0, v.shape) * interior[:, None]
    return v, c


def mesh(oracle, kind, perturb=0.1, seed=7):
    v, c = linear_mesh(oracle, GEOM[kind], perturb, seed)
    if kind == HEX27:
        return oracle.hex8_to_hex27(v, c)
    if kind == TET20:
        return oracle.tet4_to_tet20(v, c)
    if kind in (TET10, TRI6, QUAD9, HEX20):
        return oracle.refine_to_quadratic(GEOM[kind], v, c)
    return v, c


def rule(oracle, kind):
    """a rule per kind (any rule serves: the quantities are pointwise)"""
    if kind == HEX8:
        return oracle.hexahedron_gauss(2)
    if kind in (HEX27, HEX20):
        return oracle.hexahedron_gauss(3)
    if kind == QUAD4:
        return oracle.quadrilateral_gauss(2)
    if kind == QUAD9:
        return oracle.quadrilateral_gauss(3)
    if kind in (TET4, TET10, TET20):
        return oracle.tetrahedron_rule({TET4: 2, TET10: 3, TET20: 4}[kind])
    return oracle.triangle_rule(2 if kind == TRI3 else 3)


def von_mises(sg):
    if sg.shape[0] == 2:   # the in-plane form
        return np.sqrt(sg[0, 0] ** 2 - sg[0, 0] * sg[1, 1] + sg[1, 1] ** 2 + 3.0 * sg[0, 1] ** 2)
    dev = sg - np.trace(sg) / 3.0 * np.eye(3)
    return np.sqrt(1.5 * np.sum(dev * dev))


def point_quantities(oracle, op, gu, mu, lam):
    """every quantity of one point from gu[i][k] = d u_k / d x_i"""
    d = gu.shape[0]
    out = {"grad_u": gu.copy()}
    if op == LAPLACE:
        out["stress_pk1"] = gu.T.copy()
        out["energy_density"] = 0.5 * float(np.sum(gu * gu))
        return out
    F = np.eye(d) + gu.T
    P = oracle.material_stress_tensor(op, F, mu, lam)
    out["stress_pk1"] = P
    out["energy_density"] = oracle.material_energy_density(op, F, mu, lam)
    if op == LINEAR_ELASTIC:
        out["strain"] = 0.5 * (gu + gu.T)
        sg = P
    else:
        out["strain"] = 0.5 * (F.T @ F - np.eye(d))
        dF = np.linalg.det(F)
        sg = P @ F.T / dF if dF > 0.0 else np.full((d, d), np.nan)
    out["cauchy_stress"] = sg
    out["von_mises"] = von_mises(sg)
    return out


def lame_at(params, e, q):
    """params: (mu, lambda) | (nq, 2) array | (rule_params (R, nq, 2), elem_to_rule (E,))"""
    if isinstance(params, tuple) and len(params) == 2 and np.ndim(params[0]) == 3:
        return tuple(params[0][int(params[1][e]), q])
    p = np.asarray(params, dtype=np.float64)
    return tuple(p) if p.ndim == 1 else tuple(p[q])


def recover(oracle, kind, op, v, c, w, p, params, u, mask=None):
    """{quantity: {"points": (E nq, ...), "elements": (E, ...), "nodes": (N, ...)}} and "volume": (E,)"""
    v, c = np.asarray(v, dtype=np.float64), np.asarray(c).astype(np.int64)
    E, n = c.shape
    N, d = v.shape
    s = 1 if op == LAPLACE else d
    nq = len(w)
    ng = NG[GEOM[kind]]
    U = np.zeros((N, s)) if u is None else np.asarray(u, dtype=np.float64).reshape(N, s)
    G = [oracle.element_gradients(kind, p[q]) for q in range(nq)]            # (d, n): G[j, a] = d phi_a / d xi_j
    Gg = [oracle.element_gradients(GEOM[kind], p[q]) for q in range(nq)]     # (d, ng)
    active = np.ones(E, dtype=bool) if mask is None else np.asarray(mask).astype(bool)
    names = quantities_of(op)
    shapes = {"grad_u": (d, s), "strain": (d, d), "stress_pk1": (s, d), "cauchy_stress": (d, d), "von_mises": (), "energy_density": ()}
    pts = {k: np.zeros((E, nq) + shapes[k]) for k in names}
    mean = {k: np.zeros((E,) + shapes[k]) for k in names}
    vol = np.zeros(E)
    for e in range(E):
        if not active[e]:
            continue
        X = v[c[e, :ng]]
        acc = {k: np.zeros(shapes[k]) for k in names}
        for q in range(nq):
            J = X.T @ Gg[q].T                       # J[i][j] = sum_a x_a,i d phi_a / d xi_j
            R = G[q] @ U[c[e]]                      # R[j][k] = sum_a d phi_a / d xi_j u_a,k
            gu = np.linalg.inv(J).T @ R
            sq = w[q] * abs(np.linalg.det(J))
            mu, lam = (0.0, 0.0) if op == LAPLACE else lame_at(params, e, q)
            val = point_quantities(oracle, op, gu, mu, lam)
            vol[e] += sq
            for k in names:
                pts[k][e, q] = val[k]
                acc[k] = acc[k] + sq * np.asarray(val[k])
        for k in names:
            mean[k][e] = acc[k] / vol[e]
    out = {"volume": vol}
    for k in names:
        nod = np.zeros((N,) + shapes[k])
        vs = np.zeros(N)
        for e in range(E):                          # ascending element order, an element counts once per node
            if active[e]:
                for a in np.unique(c[e]):
                    nod[a] = nod[a] + vol[e] * mean[k][e]
                    vs[a] += vol[e]
        touched = np.zeros(N, dtype=bool)
        touched[np.unique(c[active])] = True
        for a in range(N):
            nod[a] = nod[a] / vs[a] if touched[a] else 0.0
        out[k] = {"points": pts[k].reshape((E * nq,) + shapes[k]), "elements": mean[k], "nodes": nod}
    return out


def affine_field(v, A, b):
    """u = A x + b at the nodes, flattened node-major; A is (s, d)"""
    return (np.asarray(v) @ np.asarray(A).T + np.asarray(b)).reshape(-1)


def affine_matrix(op, d, seed=3):
    """A with |A|_F about 0.2 and det(I + A) > 0, b"""
    rng = np.random.default_rng(seed)
    s = 1 if op == LAPLACE else d
    A = rng.uniform(-1.0, 1.0, (s, d))
    A *= 0.2 / np.linalg.norm(A)
    if s == d:
        assert np.linalg.det(np.eye(d) + A) > 0.0
    return A, rng.uniform(-1.0, 1.0, s)


def smooth_field(v, s):
    """u_k = 0.1 sin(...) at the nodes"""
    v = np.asarray(v)
    d = v.shape[1]
    k = np.arange(s)[None, :]
    ph = sum((1.0 + 0.5 * i + 0.3 * k) * v[:, [i]] for i in range(d))
    return (0.1 * np.sin(ph + 0.4 * k)).reshape(-1)
