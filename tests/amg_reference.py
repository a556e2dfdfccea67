"""A NumPy / SciPy restatement of the documented smoothed-aggregation hierarchy (pure Python, no library code): what fh_amg_create,
fh_amg_set_smoother and fh_amg_apply_dev have to compute, formula by formula.

1. Strength and aggregation: block Frobenius norms per node pair, strong = nf > 0 and nf >= theta sqrt(||A_ii||_F ||A_jj||_F), isolated =
   no nonzero off-diagonal block (whatever theta is); the distance-2 independent set by the documented priority, the join and one sweep,
   all three on the strong graph.  _strength also reports how near any link sits to the threshold, which a test has to keep away from.
2. The tentative prolongator by modified Gram-Schmidt per aggregate with the drop rule, P = (I - omega D^-1 A) T over all of A (not only its
   strong part), zero rows on isolated nodes, A_c = P^T A P.  A dropped coarse dof has a zero row and column in A_c; D^-1 = 0 there.
3. The eigenvalue estimate (`steps` Jacobi-PCG / Lanczos steps from the fixed start vector, zero on isolated nodes), the Chebyshev-Jacobi
   smoother (degree, range), the V-cycle with the isolated nodes' blocks inverted by Cholesky under the documented pivot rule, and PCG.
"""
import numpy as np
import scipy.sparse as sp


def _node_graph(A, b):
    """node graph of the nonzero off-diagonal blocks of a scalar CSR with b x b blocks"""
    Ac = abs(A).tocsr()
    Ac.eliminate_zeros()
    Ac = Ac.tocoo()
    G = sp.csr_matrix((np.ones(Ac.nnz), (Ac.row // b, Ac.col // b)), shape=(A.shape[0] // b,) * 2)
    G.setdiag(0)
    G.eliminate_zeros()
    return G


def _strength(A, b, theta):
    """(S, G, margin): the strong graph and the graph of all nonzero off-diagonal blocks (both with unit entries), and the least relative
    distance min |nf / (theta sqrt(dn_i dn_j)) - 1| of an off-diagonal block from the threshold (inf at theta = 0)"""
    Ac = A.tocoo()
    N = A.shape[0] // b
    F = sp.csr_matrix((Ac.data ** 2, (Ac.row // b, Ac.col // b)), shape=(N, N))   # (duplicates sum: squared block norms)
    dn = np.sqrt(F.diagonal())
    F.setdiag(0)
    F.eliminate_zeros()
    F = F.tocoo()
    nf = np.sqrt(F.data)
    thr = theta * np.sqrt(dn[F.row] * dn[F.col])
    strong = (nf > 0) & (nf >= thr)
    with np.errstate(divide="ignore", invalid="ignore"):
        dist = np.abs(nf / thr - 1.0)
    margin = float(np.nanmin(dist)) if len(dist) and theta > 0 else np.inf
    G = sp.csr_matrix((np.ones(len(nf)), (F.row, F.col)), shape=(N, N))
    S = sp.csr_matrix((np.ones(strong.sum()), (F.row[strong], F.col[strong])), shape=(N, N))
    return S, G, margin


def _tentative(agg, B, b, nb):
    """T and the coarse B by modified Gram-Schmidt per aggregate, with the documented drop rule"""
    N = len(agg)
    nagg = int(agg.max()) + 1 if (agg >= 0).any() else 0
    T = np.zeros((N * b, nb))
    Bc = np.zeros((nagg * nb, nb))
    order = np.argsort(agg, kind="stable")
    first = np.searchsorted(agg[order], np.arange(nagg + 1))
    for J in range(nagg):
        rows = (b * order[first[J]:first[J + 1]][:, None] + np.arange(b)).ravel()
        Q = B[rows].copy()
        Rm = np.zeros((nb, nb))
        for k in range(nb):
            n0 = np.linalg.norm(Q[:, k])
            for j in range(k):
                r = Q[:, j] @ Q[:, k]
                Q[:, k] -= r * Q[:, j]
                Rm[j, k] = r
            n1 = np.linalg.norm(Q[:, k])
            if not n1 > 1e-10 * n0:
                Q[:, k] = 0.0
            else:
                Q[:, k] /= n1
                Rm[k, k] = n1
        T[rows] = Q
        Bc[J * nb:(J + 1) * nb] = Rm
    # block column agg(i) of node i's rows
    rr = np.repeat(np.arange(N * b), nb)
    node = rr // b
    cc = np.where(agg[node] >= 0, agg[node] * nb, 0) + np.tile(np.arange(nb), N * b)
    Tf = sp.csr_matrix((T.ravel() * (agg[node] >= 0), (rr, cc)), shape=(N * b, nagg * nb))
    Tf.eliminate_zeros()
    return Tf, Bc


def _rigid(m):
    x = m.vertices - m.vertices.mean(axis=0)
    N, d = x.shape
    if d == 2:
        B = np.zeros((2 * N, 3))
        B[0::2, 0] = 1
        B[1::2, 1] = 1
        B[0::2, 2] = -x[:, 1]
        B[1::2, 2] = x[:, 0]
        return B
    B = np.zeros((3 * N, 6))
    for a in range(3):
        B[a::3, a] = 1
    B[1::3, 3], B[2::3, 3] = -x[:, 2], x[:, 1]
    B[0::3, 4], B[2::3, 4] = x[:, 2], -x[:, 0]
    B[0::3, 5], B[1::3, 5] = -x[:, 1], x[:, 0]
    return B


def _key(n):
    """the documented priority ((h(i) & 0x7fffffff) << 32) | i"""
    i = np.arange(n, dtype=np.uint64)
    m = np.uint64(0xFFFFFFFF)
    h = i.copy()
    with np.errstate(over="ignore"):
        h ^= h >> np.uint64(16)
        h = (h * np.uint64(0x7FEB352D)) & m
        h ^= h >> np.uint64(15)
        h = (h * np.uint64(0x846CA68B)) & m
        h ^= h >> np.uint64(16)
    return ((h & np.uint64(0x7FFFFFFF)) << np.uint64(32)) | i


def _rowmax(G, v):
    """max of v over each row's columns (0 for an empty row); v >= 0 and exact in float64"""
    M = G.multiply(v[None, :]).tocsr()
    return np.asarray(M.max(axis=1).toarray()).ravel()


def _np_aggregate(A, b, theta=0.0, info=None):
    """the documented aggregation: aggregates (-1: isolated) and roots.  The independent set, the join and the sweep walk the strong graph
    of `theta`; a node is isolated when it has no nonzero off-diagonal block at all.  info (a dict) receives margin (_strength), the
    numbers of strong and of weak links, and the number of one-node aggregates"""
    S, Gall, margin = _strength(A, b, theta)
    G = S
    N = G.shape[0]
    iso = np.diff(Gall.indptr) == 0
    rank = np.empty(N, dtype=np.int64)
    rank[np.argsort(_key(N))] = np.arange(N)
    state = np.where(iso, 3, 0)
    while (state == 0).any():
        v = np.where(state == 0, rank + 1.0, np.where(state == 1, N + 2.0, 0.0))
        v1 = np.maximum(v, _rowmax(G, v))
        v2 = np.maximum(v1, _rowmax(G, v1))
        und = state == 0
        state[und & (v2 == rank + 1.0)] = 1
        state[und & (v2 == N + 2.0)] = 2
    roots = np.where(state == 1)[0]
    rid = np.full(N, -1)
    rid[roots] = np.arange(len(roots))
    agg = np.full(N, -1)
    agg[roots] = rid[roots]
    Gr = G @ sp.diags((state == 1) * (rank + 1.0))
    best = _rowmax(Gr, np.ones(N))   # (the column values already carry rank + 1)
    Gr = Gr.tocsr()
    for i in np.where((state == 2) & (best > 0))[0]:
        cols = Gr.indices[Gr.indptr[i]:Gr.indptr[i + 1]]
        vals = Gr.data[Gr.indptr[i]:Gr.indptr[i + 1]]
        agg[i] = rid[cols[np.argmax(vals)]]
    agg0 = agg.copy()
    for i in np.where((agg0 < 0) & ~iso)[0]:
        cols = G.indices[G.indptr[i]:G.indptr[i + 1]]
        cols = cols[agg0[cols] >= 0]
        if not len(cols):
            raise RuntimeError("a node was left without an aggregate")
        agg[i] = agg0[cols[np.argmax(rank[cols])]]
    if info is not None:
        info.update(margin=margin, strong=S.nnz, weak=Gall.nnz - S.nnz, one_node=int((np.bincount(agg[agg >= 0]) == 1).sum()))
    return agg, roots


def _np_lambda(A, b, iso, steps=10):
    """the documented estimate: `steps` Jacobi-PCG / Lanczos steps from the fixed start vector (zero on the isolated nodes of any level)"""
    n = A.shape[0]
    with np.errstate(over="ignore"):
        h = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x632BE59BD9B4E019)
        h ^= h >> np.uint64(31)
        h *= np.uint64(0xBF58476D1CE4E5B9)
        h ^= h >> np.uint64(29)
    v = 2.0 * ((h >> np.uint64(11)).astype(np.float64) * 2.0 ** -53) - 1.0
    v[np.repeat(iso, b)] = 0.0
    d = A.diagonal()
    dinv = np.where(d != 0, 1.0 / np.where(d != 0, d, 1.0), 0.0)
    r = v.copy()
    z = dinv * r
    p = z.copy()
    zr = z @ r
    al, be = [], []
    for k in range(steps):
        if not zr > 0:
            break
        Ap = A @ p
        a = zr / (p @ Ap)
        al.append(a)
        r = r - a * Ap
        z = dinv * r
        zr1 = z @ r
        bt = zr1 / zr
        zr = zr1
        if k + 1 == steps or not zr > 0:
            break
        be.append(bt)
        p = z + bt * p
    k = len(al)
    T = np.zeros((k, k))
    for i in range(k):
        T[i, i] = 1.0 / al[i] + (be[i - 1] / al[i - 1] if i else 0.0)
        if i + 1 < k:
            T[i, i + 1] = T[i + 1, i] = np.sqrt(be[i]) / al[i]
    return float(np.linalg.eigvalsh(T).max())


def _restate(amg, B0, A0=None, b0=None, theta=0.0, steps=10, info=None):
    """per level: (A, P, T, B, Bc, agg, lambda) restated from the documented formulas.  With amg: the device's fine A, aggregates and lambda;
    with A0 (amg None): everything on the CPU (aggregation at `theta`, the eigenvalue estimate of `steps` steps), coarsening to at most 4096
    dofs.  info (a list) receives one dict per coarsened level: what _np_aggregate reports (amg None), and `dropped`, the number of
    columns the drop rule removed"""
    A = amg.level_matrix(0, "A") if amg is not None else A0
    A = A.tocsr()
    A.eliminate_zeros()
    B = B0
    b = amg.level_info(0)["block_size"] if amg is not None else b0
    out = []
    l = 0
    while (amg is not None and l < amg.num_levels - 1) or (amg is None and A.shape[0] > 4096):
        nb = B.shape[1]
        rec = {}
        if amg is not None:
            agg, lam = amg.aggregates(l), amg.level_info(l)["lambda_max"]
        else:
            agg, _ = _np_aggregate(A, b, theta, rec)
            lam = _np_lambda(A, b, agg < 0, steps)
        T, Bc = _tentative(agg, B, b, nb)
        rec["dropped"] = int((Bc.reshape(-1, nb, nb)[:, np.arange(nb), np.arange(nb)] == 0).sum())
        if info is not None:
            info.append(rec)
        d = A.diagonal()
        dinv = np.where(d != 0, 1.0 / np.where(d != 0, d, 1.0), 0.0)
        omega = 4.0 / (3.0 * lam)
        P = (T - omega * sp.diags(dinv) @ (A @ T)).tocsr()
        iso = np.repeat(agg < 0, b)
        P = (sp.diags((~iso).astype(float)) @ P).tocsr()
        out.append((A, P, T, B, Bc, agg, lam))
        A = (P.T @ (A @ P)).tocsr()
        B = Bc
        b = nb
        l += 1
    out.append((A, None, None, B, None, None, 0.0))
    return out


def _np_cheb(A, dinv, lam, b, x, zero, degree=3, rng_=15.0):
    hi, lo = 1.1 * lam, lam / rng_
    theta, delta = 0.5 * (hi + lo), 0.5 * (hi - lo)
    if zero:
        x = np.zeros_like(b)
    r = b - A @ x
    d = dinv * r / theta
    rho = delta / theta
    for k in range(1, degree + 1):
        x = x + d
        if k < degree:
            r = r - A @ d
            rho1 = 1.0 / (2.0 * theta / delta - rho)
            d = rho1 * rho * d + 2.0 * rho1 / delta * dinv * r
            rho = rho1
    return x


def _iso_inverse(M):
    """the documented inverse of an isolated node's diagonal block: Cholesky M = L L^T, W = L^-1, W^T W; a pivot at most 1e-14 of its
    diagonal entry (or a zero diagonal entry) leaves that dof out, its row and column of the result zero.  (inverse, dofs left out)"""
    R = M.shape[0]
    L = np.array(M, dtype=np.float64)
    W = np.zeros((R, R))
    out = np.zeros(R, dtype=bool)
    for j in range(R):
        d0 = L[j, j]
        sj = d0 - L[j, :j] @ L[j, :j]
        out[j] = not sj > 1e-14 * d0
        if out[j]:
            L[j:, j] = 0.0
            continue
        L[j, j] = np.sqrt(sj)
        for a in range(j + 1, R):
            L[a, j] = (L[a, j] - L[a, :j] @ L[j, :j]) / L[j, j]
    for c in range(R):
        if out[c]:
            continue
        W[c, c] = 1.0 / L[c, c]
        for a in range(c + 1, R):
            if not out[a]:
                W[a, c] = -(L[a, c:a] @ W[c:a, c]) / L[a, a]
    return W.T @ W, out


def _np_vcycle(levels, b, l=0, degree=3, rng_=15.0):
    """the documented V-cycle on restated levels"""
    A = levels[l][0]
    if l == len(levels) - 1:
        Ad = A.toarray()
        act = np.diag(Ad) != 0
        x = np.zeros_like(b)
        x[act] = np.linalg.solve(Ad[np.ix_(act, act)], b[act])
        return x
    P, agg, lam = levels[l][1], levels[l][5], levels[l][6]
    bs = A.shape[0] // len(agg)
    d = A.diagonal()
    dinv = np.where(d != 0, 1.0 / np.where(d != 0, d, 1.0), 0.0)
    x = _np_cheb(A, dinv, lam, b, None, True, degree, rng_)
    xc = _np_vcycle(levels, P.T @ (b - A @ x), l + 1, degree, rng_)
    x = x + P @ xc
    x = _np_cheb(A, dinv, lam, b, x, False, degree, rng_)
    nodes = np.where(agg < 0)[0]   # isolated nodes: A_ii^-1 b_i by the pivot-rule inverse
    for i, M in zip(nodes, _diagonal_blocks(A, nodes, bs)):
        rows = slice(bs * i, bs * (i + 1))
        x[rows] = _iso_inverse(M)[0] @ b[rows]
    return x


def _diagonal_blocks(A, nodes, bs):
    """the dense bs x bs diagonal blocks of the given nodes"""
    out = np.zeros((len(nodes), bs, bs))
    if len(nodes):
        dofs = (bs * nodes[:, None] + np.arange(bs)).ravel()
        M = A[dofs].tocoo()
        own = M.col // bs == nodes[M.row // bs]
        out[M.row[own] // bs, M.row[own] % bs, M.col[own] % bs] = M.data[own]
    return out


def _np_pcg(levels, b, tol=1e-8, degree=3, rng_=15.0):
    """PCG with the restated V-cycle, as fh_cg_solve runs it: the iteration count"""
    A = levels[0][0]
    x = np.zeros_like(b)
    r = b.copy()
    z = _np_vcycle(levels, r, 0, degree, rng_)
    p = z.copy()
    zr = z @ r
    bn = np.linalg.norm(b)
    it = 0
    while np.linalg.norm(r) > tol * bn:
        Ap = A @ p
        a = zr / (p @ Ap)
        x += a * p
        r -= a * Ap
        it += 1
        z = _np_vcycle(levels, r, 0, degree, rng_)
        zr1 = z @ r
        p = z + (zr1 / zr) * p
        zr = zr1
        if it > 500:
            break
    return it
