"""Crafted node-blocked CSR patterns and plain references for the kernels that walk them (pure Python / numpy / scipy, no library code).

1. Patterns from ragged element lists: stars (one hub row of k blocks, leaves of 2), cliques (every row k blocks), rows of one block and of
   none, chains that pad the node count.  Every generator also states the row lengths it means to produce; node_pattern() derives them again
   from the incidence matrix (inc^T inc), which is what the library's pattern has to equal.
2. The value layout of the library (global.rs:100-118): the S scalar rows of a node are contiguous, each S * cnt long, and share the node's
   ascending column list -- which is plain CSR with sorted indices over scalar_pattern()'s arrays.
3. References: integer SpMV in int64 (exact), real SpMV in np.longdouble with the |A||x| of the error bound, the same in fractions.Fraction
   for a small case, and one step of (preconditioned) conjugate gradients from exact integer sums.
"""
from fractions import Fraction

import numpy as np

LD = np.longdouble
EXACT = 1 << 53            # integers below this are doubles, and so is every sum of them that stays below it


# ------------------------------------------------------------------------------------------------------------------ patterns
class Pattern:
    """num_nodes, the ragged element lists, and the number of column blocks each node row is meant to have"""

    def __init__(self, name, num_nodes, elements, counts):
        self.name, self.num_nodes, self.elements, self.counts = name, num_nodes, elements, np.asarray(counts, dtype=np.int64)
        assert len(self.counts) == num_nodes

    @property
    def max_row(self):
        return int(self.counts.max())

    def __repr__(self):
        return self.name


def star(k):
    """elements [0, j], j = 1 .. k-1: the hub row has k blocks, the leaves 2"""
    assert k >= 2
    return Pattern(f"star{k}", k, [[0, j] for j in range(1, k)], [k] + [2] * (k - 1))


def clique(k):
    """one element of k nodes: every row has k blocks"""
    return Pattern(f"clique{k}", k, [list(range(k))], [k] * k)


def with_single(p):
    """one more node in an element of its own: a row of one block"""
    n = p.num_nodes
    return Pattern(p.name + "+single", n + 1, p.elements + [[n]], list(p.counts) + [1])


def with_isolated(p):
    """one more node in no element: a row of no blocks"""
    return Pattern(p.name + "+isolated", p.num_nodes + 1, list(p.elements), list(p.counts) + [0])


def with_chain(p, num_nodes):
    """2-node elements [i, i+1] from p's last node on, up to num_nodes nodes in all"""
    n = p.num_nodes
    assert num_nodes >= n and p.counts[n - 1] >= 1
    if num_nodes == n:
        return Pattern(f"{p.name}+pad{num_nodes}", n, list(p.elements), p.counts)
    counts = list(p.counts)
    counts[n - 1] += 1
    counts += [3] * (num_nodes - n - 1) + [2]
    return Pattern(f"{p.name}+pad{num_nodes}", num_nodes, p.elements + [[i, i + 1] for i in range(n - 1, num_nodes - 1)], counts)


def padded(num_nodes):
    """a small star (at most 9 nodes) padded with a chain to num_nodes nodes; one node: an element of its own"""
    if num_nodes == 1:
        return Pattern("single", 1, [[0]], [1])
    return with_chain(star(min(num_nodes, 9)), num_nodes)


def node_pattern(p):
    """(noff, ncols) of the node-level pattern from the incidence matrix: row i holds the nodes that share an element with i, ascending"""
    import scipy.sparse as sp

    lens = [len(e) for e in p.elements]
    rows = np.repeat(np.arange(len(p.elements)), lens)
    cols = np.array([x for e in p.elements for x in e], dtype=np.int64)
    inc = sp.csr_matrix((np.ones(len(cols), dtype=np.int64), (rows, cols)), shape=(len(p.elements), p.num_nodes))
    adj = (inc.T @ inc).tocsr()
    adj.sort_indices()
    assert adj.data.min(initial=1) >= 1
    return adj.indptr.astype(np.int64), adj.indices.astype(np.int64)


def scalar_pattern(noff, ncols, S):
    """(row_offsets, col_indices) of the scalar CSR: rows S i + a (a < S), each the S cnt_i columns S j + c (c < S) over the node's columns j"""
    cnt = np.diff(noff)
    row_len = np.repeat(S * cnt, S)
    ro = np.concatenate([[0], np.cumsum(row_len)]).astype(np.int64)
    block_cols = (S * ncols[:, None] + np.arange(S)[None, :]).reshape(-1)      # the scalar columns of node row i: [S noff_i, S noff_{i+1})
    start = np.repeat(S * noff[:-1], S)
    idx = np.repeat(start - ro[:-1], row_len) + np.arange(ro[-1])
    return ro, block_cols[idx].astype(np.int64)


def scalar_pattern_naive(noff, ncols, S):
    """the same, written as the loops of the layout's definition"""
    ro, ci = [0], []
    for i in range(len(noff) - 1):
        for a in range(S):
            for k in range(noff[i], noff[i + 1]):
                ci += [S * ncols[k] + c for c in range(S)]
            ro.append(len(ci))
    return np.array(ro, dtype=np.int64), np.array(ci, dtype=np.int64)


def row_of_entry(ro):
    return np.repeat(np.arange(len(ro) - 1), np.diff(ro))


def diagonal_positions(ro, ci):
    """index of the entry (r, r) in the value array for every scalar row r, -1 where the row has none"""
    rows = row_of_entry(ro)
    pos = np.full(len(ro) - 1, -1, dtype=np.int64)
    hit = np.nonzero(ci == rows)[0]
    pos[rows[hit]] = hit
    return pos


def to_scipy(ro, ci, values):
    import scipy.sparse as sp

    n = len(ro) - 1
    return sp.csr_matrix((values, ci, ro), shape=(n, n))


# ------------------------------------------------------------------------------------------------------------------ SpMV
def spmv_int(ro, ci, values, x):
    """A x in int64 for integer-valued double arrays; also max_i (|A||x|)_i, the bound on every partial sum"""
    a = to_scipy(ro, ci, values.astype(np.int64))
    xi = x.astype(np.int64)
    return a @ xi, int((abs(a) @ np.abs(xi)).max(initial=0))


def _row_sums(ro, terms):
    out = np.zeros(len(ro) - 1, dtype=terms.dtype)
    full = np.diff(ro) > 0
    if full.any():
        out[full] = np.add.reduceat(terms, ro[:-1][full])     # (reduceat over the non-empty rows only: an empty one would take its neighbour's entry)
    return out


def spmv_longdouble(ro, ci, values, x):
    """(A x, |A||x|) in np.longdouble"""
    terms = values.astype(LD) * x.astype(LD)[ci]
    return _row_sums(ro, terms), _row_sums(ro, np.abs(terms))


def spmv_fraction(ro, ci, values, x):
    """(A x, |A||x|) exactly"""
    y, ay = [], []
    for r in range(len(ro) - 1):
        terms = [Fraction(float(values[k])) * Fraction(float(x[ci[k]])) for k in range(ro[r], ro[r + 1])]
        y.append(sum(terms, Fraction(0)))
        ay.append(sum((abs(t) for t in terms), Fraction(0)))
    return y, ay


# ------------------------------------------------------------------------------------------------------------------ value arrays
def integer_values(rng, nnz, bound):
    return rng.integers(-bound, bound + 1, size=nnz).astype(np.float64)


def scaled_normals(rng, n):
    """standard normals times 10^u, u uniform in [-6, 6], per entry"""
    return rng.standard_normal(n) * 10.0 ** rng.uniform(-6.0, 6.0, n)


def dominant_integer_values(rng, ro, ci, power_of_two_diagonal):
    """Independent integers in [-3, 3] everywhere off the scalar diagonal (so neither the matrix nor its S x S blocks are symmetric); the
    diagonal entry of row r exceeds both the absolute off-diagonal sum of row r and that of column r, so the symmetric part is strictly
    diagonally dominant and p . A p > 0.  power_of_two_diagonal: the entries are 2^e_r, the exponents e_r differing between neighbouring rows
    (and so between the S components of a node) and spanning DIAG_SPAN + 1 values.  -> (values, exponents or None)"""
    n = len(ro) - 1
    values = integer_values(rng, len(ci), 3)
    dpos = diagonal_positions(ro, ci)
    assert (dpos >= 0).all(), "a row without a diagonal entry"
    values[dpos] = 0.0
    av = np.abs(values)
    bound = np.maximum(_row_sums(ro, av), np.bincount(ci, weights=av, minlength=n)).astype(np.int64)
    if not power_of_two_diagonal:
        values[dpos] = (bound + 1 + rng.integers(0, 3, size=n)).astype(np.float64)
        return values, None
    e0 = int(bound.max() + 1).bit_length()            # 2^e0 > max bound
    r = np.arange(n)
    e = e0 + (r + r // 7) % (DIAG_SPAN + 1)           # rows r, r+1, r+2 never share an exponent
    values[dpos] = np.ldexp(1.0, e)
    return values, e.astype(np.int64)


DIAG_SPAN = 3


def cg_first_step(ro, ci, values, b, exponents=None):
    """The iterate after one CG step from x0 = 0 with integer A and b, identity (exponents None) or Jacobi preconditioner with the diagonal
    2^exponents.  With z = D^-1 b:  alpha = fl((z . b) / (z . A z)),  x1 = fl(alpha z).  Everything before the division is formed in integers:
    with E = max exponent, Z = 2^E z is an integer vector, z . b = 2^-E (Z . b) and z . A z = 2^-2E (Z . A Z).

    -> (x1, budget): budget is the largest integer any partial sum of the three dot products and of the products A z can reach in those
    units (sums of absolute values), whatever the order of summation; below 2^53 every one of them is exact in doubles -- including the
    device's fused multiply-adds, whose exact results need no rounding."""
    a = to_scipy(ro, ci, values.astype(np.int64))
    bi = b.astype(np.int64)
    if exponents is None:
        emax, shift = 0, np.zeros(len(bi), dtype=np.int64)
    else:
        emax = int(exponents.max())
        shift = emax - exponents
        assert np.array_equal(values[diagonal_positions(ro, ci)], np.ldexp(1.0, exponents))
    Z = bi << shift
    AZ = a @ Z
    absAZ = abs(a) @ np.abs(Z)
    zb, zAz = int(np.dot(Z, bi)), int(np.dot(Z, AZ))
    budget = max(int(np.dot(np.abs(Z), np.abs(bi))), int(np.dot(bi, bi)), int(absAZ.max()), int(np.dot(np.abs(Z), absAZ)))
    # (int64 holds these: |Z| < 2^12, |A| < 2^20, fewer than 2^19 rows of fewer than 2^12 entries)
    assert zAz > 0 and zb > 0
    if budget >= EXACT:
        return None, budget
    alpha = np.ldexp(float(zb), -emax) / np.ldexp(float(zAz), -2 * emax)
    z = np.ldexp(b, -exponents) if exponents is not None else b
    return alpha * z, budget


def symmetric_dominant_values(rng, ro, ci):
    """real symmetric strictly diagonally dominant values on a structurally symmetric pattern (an SPD matrix)"""
    n = len(ro) - 1
    a = to_scipy(ro, ci, rng.uniform(-1.0, 1.0, len(ci)))
    a = (a + a.T).tocsr()
    a.sort_indices()
    assert np.array_equal(a.indptr, ro) and np.array_equal(a.indices, ci)
    values = a.data.copy()
    dpos = diagonal_positions(ro, ci)
    values[dpos] = 0.0
    values[dpos] = _row_sums(ro, np.abs(values)) * rng.uniform(1.05, 1.5, n) + rng.uniform(0.5, 1.0, n)
    return values


# ------------------------------------------------------------------------------------------------------------------ Dirichlet
def dirichlet_rhs(v, nodes, S):
    out = v.copy()
    out.reshape(-1, S)[np.asarray(nodes, dtype=np.int64)] = 0.0
    return out
