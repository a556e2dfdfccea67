"""Host model of Dirichlet conditions on single components (fh_set_operator_dirichlet_dofs, fh_apply_dirichlet_dofs_*): the constrained
matrix is K with the rows and columns of the constrained dofs zeroed and `scale` on their diagonal, scale = |first nonzero diagonal entry of
K| in row order, or 1 -- what apply_homogeneous_dirichlet_bc_csr leaves for a node set, per dof.  Numpy only."""
import numpy as np
import scipy.sparse as sp


def dof_list(nodes, masks, s):
    """sorted unique dofs s node + j with bit j of the node's (OR-ed) mask set"""
    out = set()
    for nd, mk in zip(np.asarray(nodes, dtype=np.int64), np.asarray(masks, dtype=np.int64)):
        out.update(int(nd) * s + j for j in range(s) if (mk >> j) & 1)
    return np.array(sorted(out), dtype=np.int64)


def scale_of(K):
    d = np.asarray(K.diagonal()).reshape(-1)
    nz = np.nonzero(d)[0]
    return abs(float(d[nz[0]])) if len(nz) else 1.0


def constrain(K, dofs, scale=None):
    """the constrained matrix (dense); scale None: from K"""
    A = np.array(K.toarray() if sp.issparse(K) else K, dtype=np.float64)
    scale = scale_of(A) if scale is None else scale
    A[dofs, :] = 0.0
    A[:, dofs] = 0.0
    A[dofs, dofs] = scale
    return A


def eliminate(K, dofs, b):
    """x with K_ff x_f = b_f on the free dofs and x = 0 on the constrained ones: dense elimination"""
    A = np.array(K.toarray() if sp.issparse(K) else K, dtype=np.float64)
    free = np.ones(len(A), dtype=bool)
    free[dofs] = False
    x = np.zeros(len(A))
    x[free] = np.linalg.solve(A[free][:, free], np.asarray(b, dtype=np.float64)[free])
    return x


def random_mixed_set(rng, num_nodes, s):
    """about a third of the nodes, in random order: fully constrained ones, ones with one component and (s >= 2) ones with two (s >= 3: so
    partly constrained in two ways); s = 1: bit 0 only"""
    nodes = rng.permutation(num_nodes)[:max(3, num_nodes // 3)]
    masks = np.zeros(len(nodes), dtype=np.uint8)
    for k in range(len(nodes)):
        how = k % 3
        if s == 1 or how == 0:
            masks[k] = (1 << s) - 1
        elif how == 1 or s == 2:
            masks[k] = 1 << int(rng.integers(s))
        else:
            masks[k] = ((1 << s) - 1) & ~(1 << int(rng.integers(s)))
    return nodes.astype(np.uint64), masks


# ------------------------------------------------------------------------------------------ a small K of its own (no device)
def hex8_box_elastic(res, lam, mu):
    """(vertices, connectivity, dense K) of linear elasticity on the unit cube with res^3 trilinear cells, 2 x 2 x 2 Gauss"""
    g = np.linspace(0.0, 1.0, res + 1)
    X = np.array([[x, y, z] for z in g for y in g for x in g])
    idx = lambda i, j, k: (k * (res + 1) + j) * (res + 1) + i
    corners = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)]
    conn = np.array([[idx(i + a, j + b, k + c) for a, b, c in corners] for k in range(res) for j in range(res) for i in range(res)])
    sign = 2.0 * np.array(corners) - 1.0
    gp = np.array([[a, b, c] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)]) / np.sqrt(3.0)
    h = 1.0 / res
    C = np.zeros((6, 6))
    C[:3, :3] = lam
    C[np.arange(3), np.arange(3)] += 2.0 * mu
    C[np.arange(3, 6), np.arange(3, 6)] = mu
    Ke = np.zeros((24, 24))
    for xi in gp:
        dN = np.array([[sign[a, d] * np.prod([1.0 + sign[a, e] * xi[e] for e in range(3) if e != d]) / 8.0 for d in range(3)] for a in range(8)])
        dN *= 2.0 / h   # (the cells are cubes of edge h)
        B = np.zeros((6, 24))
        for a in range(8):
            gx, gy, gz = dN[a]
            B[:, 3 * a:3 * a + 3] = [[gx, 0, 0], [0, gy, 0], [0, 0, gz], [gy, gx, 0], [0, gz, gy], [gz, 0, gx]]
        Ke += B.T @ C @ B * (h / 2.0) ** 3
    n = 3 * len(X)
    K = np.zeros((n, n))
    for el in conn:
        d = (3 * el[:, None] + np.arange(3)).ravel()
        K[np.ix_(d, d)] += Ke
    return X, conn, K


# ------------------------------------------------------------------------------------------ finite-strain uniaxial stretch
def neo_hookean_lateral_stretch(l1, mu, lam):
    """l2 with P_22(diag(l1, l2, l2)) = 0 for P = mu (F - F^-T) + lam ln(J) F^-T, by bisection"""
    p22 = lambda l2: mu * (l2 - 1.0 / l2) + lam * np.log(l1 * l2 * l2) / l2
    lo, hi = 0.3, 1.5
    assert p22(lo) < 0.0 < p22(hi)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if p22(mid) < 0.0 else (lo, mid)
    return 0.5 * (lo + hi)


# ------------------------------------------------------------------------------------------ the stepping model
class LinearProblem:
    """M a + K u = lf_n f with constrained dofs, in the shape tests/dynamics_reference.py steps (central_difference, implicit): K and M the
    assembled matrices (scipy), `fixed` the constrained dofs"""

    def __init__(self, K, M, fixed, f=None, load_factor=None):
        self.K, self.M = sp.csr_matrix(K), sp.csr_matrix(M)
        self.n = self.K.shape[0]
        self.free = np.ones(self.n, dtype=bool)
        self.free[np.asarray(fixed, dtype=np.int64)] = False
        self.f = np.zeros(self.n) if f is None else np.asarray(f, dtype=np.float64).reshape(-1)
        self.load_factor = None if load_factor is None else np.asarray(load_factor, dtype=np.float64)

    def lf(self, n):
        return 1.0 if self.load_factor is None else float(self.load_factor[min(n, len(self.load_factor) - 1)])

    def residual(self, u):
        return self.K @ u

    def energy(self, u):
        return 0.5 * float(u @ (self.K @ u))

    def tangent(self, u):
        return self.K

    def mass(self):
        return self.M

    def lumped(self):
        return np.asarray(self.M @ np.ones(self.n)).reshape(-1)

    def solve_free(self, A, b):
        fr = self.free
        x = np.zeros(self.n)
        x[fr] = np.linalg.solve(A[fr][:, fr].toarray(), b[fr])
        return x
