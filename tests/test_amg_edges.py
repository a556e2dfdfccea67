"""Smoothed-aggregation AMG off its main path: a strength threshold theta > 0 (scalar and block matrices, on every level), aggregates with
fewer rows than near-nullspace columns (the drop rule and the zero diagonals it leaves), isolated nodes with full and with rank-deficient
diagonal blocks, an isolated node on a coarse level, the smoother's parameters, and refused creates.  The reference is the NumPy
restatement of amg_reference.py; the unmarked tests pin that restatement on matrices built with SciPy alone, the gpu tests compare the
device with it at the tolerances of test_amg.py::test_parity_with_numpy (aggregates equal; T, P, A_c and B_c at 1e-12; lambda at 1e-8;
one V-cycle at 1e-11).

Measured on the MI355X (dofs per level; largest relative deviation of T, B_c, lambda, P, A_c, V-cycle; AMG-PCG device / NumPy):
  quad4 64, 0.6 y^1.05, theta 0.1     4225, 405           0, 0, 7e-15, 1e-16, 2e-16, 1e-14   13 / 13 (theta 0: 15)   margin 6.5e-3
  quad4 64, 0.1 y^1.05, theta 0.25    4225, 1158          0, 0, 8e-15, 6e-17, 3e-16, 5e-13   21 / 21 (theta 0: 68)   margin 1.9e-4
  hex8 16, 0.1 z, theta 0.25          4913, 1225          0, 0, 4e-15, 4e-17, 5e-16, 4e-13   23 / 23 (theta 0: 65)   margin 1.5e-2
  quad4 128, 0.1 y^1.05, theta 0.25   16641, 4594, 1309   0, 0, 5e-15, 2e-16, 7e-16, 3e-12   margins 9.6e-5, 2.6e-2; 3 one-node aggregates on level 1
  hex8 12 elastic, 27 weakened        6591, 534           8e-16, 1e-15, 5e-15, 9e-16, 1e-15, 3e-15   11 / 11   27 one-node aggregates, 81 dropped
  hex8 17 Laplace, nb = 6             5832, 816           2e-14, 9e-16, 3e-15, 3e-14, 4e-14, 2e-15   7 / 7     136 aggregates, 136 dropped
  hex8 12 elastic, 30 cut out         6591, 342           1e-15, 1e-15, 3e-16, 1e-15, 2e-15, 1e-15   11 / 11   cond 3.1: the 1e-11 applies
  hex8 30 elastic + 1 element         89397, 4164, 84     3e-15, 6e-15, 7e-15, 3e-15, 4e-15, 1e-14   17        coarse node 693 isolated
  smoother (1, 4, 5), (5, 30, 20)     5832, 136 / 5618, 651   lambda 8e-15, P 1e-15, A_c 2e-15, V-cycle 4e-14; both ways bitwise equal
  refresh with 2 A at theta 0.25      P bitwise equal, A_c = 2 A_c exactly"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.csgraph as csg

import fenris_amd as fa
from fenris_amd import _ffi

import amg_reference as ar
from test_amg import RULES, _mesh, _rel, _system, engine_spmv_residual

FH_BAD_ARGUMENT, FH_UNSUPPORTED = 2, 6
EPS = np.finfo(np.float64).eps
MARGIN = 1e-6   # nearer to the threshold than this, the kernel's order of summation may legitimately flip a link


@pytest.fixture()
def engine():
    eng = fa.Engine(0)
    yield eng
    eng.close()


# ------------------------------------------------------------------------------------------------ matrices built with SciPy alone
def _stencil(shape, coeffs):
    """the 5-point (2D) or 7-point (3D) anisotropic Laplacian sum_a coeffs[a] (-d^2 / dx_a^2), Dirichlet ends; node index x-fastest"""
    A = sp.csr_matrix((int(np.prod(shape)),) * 2)
    for a, (n, c) in enumerate(zip(shape, coeffs)):
        t = sp.diags([-np.ones(n - 1), 2.0 * np.ones(n), -np.ones(n - 1)], [-1, 0, 1])
        A = A + c * sp.kron(sp.identity(int(np.prod(shape[a + 1:]))), sp.kron(t, sp.identity(int(np.prod(shape[:a])))))
    return A.tocsr()


M3 = np.array([[4.0, 1.0, 0.5], [1.0, 3.0, -1.0], [0.5, -1.0, 5.0]])   # SPD


def _weaken(A, b, nodes, eps):
    """D A D with D = eps on the dofs of `nodes` (pairwise non-adjacent), then their diagonal blocks put back: E A E plus a positive
    semidefinite block diagonal, so SPD like A and on its pattern.  (D A D alone leaves ||A_ij|| / sqrt(||A_ii|| ||A_jj||) as it was.)"""
    A = A.tocoo()
    inn = np.isin(A.row // b, nodes)
    inc = np.isin(A.col // b, nodes)
    assert not (inn & inc & (A.row // b != A.col // b)).any()
    return sp.csr_matrix((np.where(inn ^ inc, eps, 1.0) * A.data, (A.row, A.col)), shape=A.shape)


def _spread_nodes(G, candidates, count, seed):
    """`count` of the candidate nodes, pairwise non-adjacent in G, by a fixed seed; ascending"""
    rng = np.random.default_rng(seed)
    chosen, blocked = [], np.zeros(G.shape[0], dtype=bool)
    for i in rng.permutation(candidates):
        if len(chosen) == count:
            break
        if not blocked[i]:
            chosen.append(i)
            blocked[i] = True
            blocked[G.indices[G.indptr[i]:G.indptr[i + 1]]] = True
    assert len(chosen) == count
    return np.sort(np.array(chosen))


def _cpu_cases():
    """(name, A, b, B0, theta): a 70 x 70 5-point stencil with weak y links; a 12^3 7-point stencil with weak z links times a 3 x 3 SPD block,
    40 of its nodes weakened into one-node aggregates (3 rows, 6 near-nullspace columns)"""
    A2 = _stencil((70, 70), (1.0, 0.05))
    yield "5-point", A2, 1, np.ones((A2.shape[0], 1)), 0.25
    L3 = _stencil((12, 12, 12), (1.0, 0.7, 0.04))
    N = L3.shape[0]
    nodes = _spread_nodes(ar._node_graph(L3, 1), np.arange(N), 40, 11)
    A3 = _weaken(sp.kron(L3, M3).tocsr(), 3, nodes, 1e-3)
    x = np.stack(np.unravel_index(np.arange(N), (12, 12, 12))[::-1], axis=1) / 11.0 - 0.5
    B0 = np.zeros((3 * N, 6))
    for a in range(3):
        B0[a::3, a] = 1.0
        B0[a::3, 3 + a] = x[:, a] + 0.25 * x[:, (a + 1) % 3]
    yield "7-point blocks", A3, 3, B0, 0.1


CPU_CASES = {c[0]: c for c in _cpu_cases()}
_restated = {}


def _cpu_levels(name):
    """the restated hierarchy of a CPU case, computed once and left unchanged: (levels, info)"""
    if name not in _restated:
        _, A, b, B0, theta = CPU_CASES[name]
        info = []
        _restated[name] = (ar._restate(None, B0, A0=A, b0=b, theta=theta, info=info), info)
    return _restated[name]


# ------------------------------------------------------------------------------------------------ the restatement, on the CPU
def test_theta_zero_is_the_pattern():
    """at theta = 0 the strong graph is the graph of the nonzero off-diagonal blocks, and the aggregation is the one of that graph"""
    _, A, b, _, _ = CPU_CASES["7-point blocks"]
    S, G, margin = ar._strength(A, b, 0.0)
    assert (S != G).nnz == 0 and (G.astype(bool) != ar._node_graph(A, b).astype(bool)).nnz == 0 and margin == np.inf
    info = {}
    agg, roots = ar._np_aggregate(A, b, info=info)
    assert info["weak"] == 0 and (agg >= 0).all() and np.array_equal(agg[roots], np.arange(len(roots)))


@pytest.mark.parametrize("name", list(CPU_CASES))
def test_restated_aggregation_walks_the_strong_graph(name):
    _, A, b, _, theta = CPU_CASES[name]
    info = {}
    agg, roots = ar._np_aggregate(A, b, theta, info)
    S, G, margin = ar._strength(A, b, theta)
    assert margin >= MARGIN and info["weak"] > 0 and info["strong"] > 0 and (S != S.T).nnz == 0
    assert (agg >= 0).all()   # (no node without an off-diagonal block)
    nagg = agg.max() + 1
    assert np.array_equal(np.unique(agg), np.arange(nagg)) and np.array_equal(agg[roots], np.arange(nagg))
    # every aggregate is connected in the strong graph: the strong links inside aggregates have as many components as there are aggregates
    Sc = S.tocoo()
    inside = agg[Sc.row] == agg[Sc.col]
    ncomp, lab = csg.connected_components(sp.csr_matrix((np.ones(inside.sum()), (Sc.row[inside], Sc.col[inside])), shape=S.shape), directed=False)
    assert ncomp == nagg and len(np.unique(nagg * lab + agg)) == nagg
    # roots are pairwise at strong distance >= 3
    S2 = (S @ S + S).tocsr()
    near = S2[roots][:, roots].tocsr()
    near.setdiag(0)
    near.eliminate_zeros()
    assert near.nnz == 0
    # no aggregate spans a weak-only link
    W = (G - S).tocoo()
    assert W.nnz == info["weak"] and not (agg[W.row] == agg[W.col]).any()
    if name == "7-point blocks":
        assert info["one_node"] >= 40   # the weakened nodes: nonzero blocks, no strong link
    else:
        assert np.bincount(agg).max() <= 5 and info["one_node"] == 0   # (pieces of x lines)


@pytest.mark.parametrize("name", list(CPU_CASES))
def test_restated_transfer(name):
    """T B_c = B, orthonormal kept columns, zero dropped ones; A_c symmetric with zero rows and columns at the dropped dofs"""
    levels, info = _cpu_levels(name)
    assert len(levels) >= 2
    dropped_seen = 0
    for l, (A, P, T, B, Bc, agg, lam) in enumerate(levels[:-1]):
        b, nb = A.shape[0] // len(agg), B.shape[1]
        on = np.repeat(agg >= 0, b)
        assert np.abs((T @ Bc)[on] - B[on]).max() <= 1e-13 * max(1.0, np.abs(B).max())
        Rm = Bc.reshape(-1, nb, nb)
        drop = Rm[:, np.arange(nb), np.arange(nb)] == 0            # (aggregate, column)
        dropped_seen += int(drop.sum())
        Gm = (T.T @ T).toarray()
        keep = ~drop.ravel()
        assert np.abs(Gm - np.diag(keep.astype(float))).max() <= 1e-13   # (columns of different aggregates share no row)
        assert abs(T[:, np.where(~keep)[0]]).sum() == 0
        # a dropped column's row of B_c is zero (its column keeps the projections that T B_c = B needs)
        assert not Rm[drop].any()
        Ac = levels[l + 1][0]
        assert abs(Ac - Ac.T).max() <= 1e-13 * abs(Ac).max()
        dead = np.where(~keep)[0]
        assert abs(Ac[dead]).sum() == 0 and abs(Ac[:, dead]).sum() == 0
        assert (Ac.diagonal()[keep] > 0).all()
    if name == "7-point blocks":
        assert info[0]["dropped"] == dropped_seen >= 3 * 40   # three rows cannot carry six columns
    else:
        assert dropped_seen == 0


def test_pivot_rule_inverse():
    rng = np.random.default_rng(17)
    for R in (3, 6):
        X = rng.standard_normal((R, R + 2))
        M = X @ X.T
        inv, out = ar._iso_inverse(M)
        ref = np.linalg.inv(M)
        assert not out.any() and np.array_equal(inv, inv.T)
        assert np.linalg.norm(inv - ref) <= 50 * np.linalg.cond(M) * EPS * np.linalg.norm(ref)
        b = rng.standard_normal(R)
        assert np.linalg.norm(inv @ b - np.linalg.solve(M, b)) <= 50 * np.linalg.cond(M) * EPS * np.linalg.norm(np.linalg.solve(M, b))
    # a Dirichlet node's block, as the present tests have them
    inv, out = ar._iso_inverse(4.0 * np.eye(3))
    assert not out.any() and np.array_equal(inv, np.eye(3) / 4.0)
    # one exactly dependent row: the inverse of the kept principal submatrix (its pseudo-inverse), zero rows and columns at the dof left out
    Lf = np.array([[2.0, 0.0, 0.0], [1.0, 3.0, 0.0], [2.0, 3.0, 0.0]])   # 3 x 3 of rank 2, the last pivot exactly zero
    X = rng.integers(-3, 4, (5, 5)).astype(float)
    E = np.zeros((6, 5))
    E[[0, 1, 3, 4, 5], np.arange(5)] = 1.0
    E[2, :2] = 1.0, -2.0                                                  # 6 x 6: row 2 = row 0 - 2 row 1, in small integers
    for M, dep in ((Lf @ Lf.T, 2), (E @ (X @ X.T + 5.0 * np.eye(5)) @ E.T, 2)):
        assert np.linalg.matrix_rank(M) == len(M) - 1
        inv, out = ar._iso_inverse(M)
        kept = np.arange(len(M)) != dep
        assert np.array_equal(out, ~kept) and np.array_equal(inv, inv.T)
        ref = np.zeros_like(M)
        ref[np.ix_(kept, kept)] = np.linalg.pinv(M[np.ix_(kept, kept)])
        assert np.linalg.norm(inv - ref) <= 50 * np.linalg.cond(M[np.ix_(kept, kept)]) * EPS * np.linalg.norm(ref)
        assert not inv[dep].any() and not inv[:, dep].any()
    # a zero diagonal entry leaves that dof out
    inv, out = ar._iso_inverse(np.diag([4.0, 0.0, 16.0]))
    assert np.array_equal(out, [False, True, False]) and np.array_equal(inv, np.diag([0.25, 0.0, 0.0625]))


@pytest.mark.parametrize("name", list(CPU_CASES))
@pytest.mark.parametrize("degree,rng_", [(3, 15.0), (1, 4.0)])
def test_restated_vcycle_is_a_preconditioner(name, degree, rng_):
    """symmetric, positive, and a contraction of the error in the A-norm"""
    _, A, b, _, _ = CPU_CASES[name]
    levels, _ = _cpu_levels(name)
    rng = np.random.default_rng(23)
    x, y = rng.standard_normal((2, A.shape[0]))
    Bx, By = (ar._np_vcycle(levels, v, 0, degree, rng_) for v in (x, y))
    p, q = x @ By, y @ Bx
    assert abs(p - q) <= 1e-12 * max(abs(p), abs(q))
    assert x @ Bx > 0 and y @ By > 0
    for e in (x, y):
        e1 = e - ar._np_vcycle(levels, A @ e, 0, degree, rng_)
        assert e1 @ (A @ e1) < e @ (A @ e)


def test_restated_smoother_parameters_matter():
    """eig_steps changes lambda, degree and range change the cycle: a parity test at other values than the defaults can fail"""
    _, A, b, _, _ = CPU_CASES["5-point"]
    levels, _ = _cpu_levels("5-point")
    iso = np.zeros(A.shape[0] // b, dtype=bool)
    l5, l10, l20 = (ar._np_lambda(A, b, iso, steps) for steps in (5, 10, 20))
    assert l5 < l10 < l20 and l10 == levels[0][6] and l20 - l5 > 1e-4 * l20
    r = np.random.default_rng(1).standard_normal(A.shape[0])
    z = ar._np_vcycle(levels, r)
    for degree, rng_ in ((1, 15.0), (3, 4.0), (5, 30.0)):
        assert np.linalg.norm(ar._np_vcycle(levels, r, 0, degree, rng_) - z) > 1e-3 * np.linalg.norm(z)


# ------------------------------------------------------------------------------------------------ the device against the restatement
def _values_on_pattern(csr, s, edit):
    """edit(values, row node, column node, row component, column component) on a host copy of the device values, written back"""
    import torch

    v = csr.values.cpu().numpy().copy()
    ro, ci = csr.row_offsets.astype(np.int64), csr.col_indices.astype(np.int64)
    rows = np.repeat(np.arange(len(ro) - 1), np.diff(ro))
    edit(v, rows // s, ci // s, rows % s, ci % s)
    csr.values.copy_(torch.from_numpy(v))


def _rhs(n, s, zero_nodes):
    import torch

    b = torch.ones(n, dtype=torch.float64, device="cuda")
    b[torch.from_numpy((s * np.asarray(zero_nodes, dtype=np.int64)[:, None] + np.arange(s)).ravel()).cuda()] = 0.0
    return b


def _parity(amg, B0, theta=0.0, steps=10, degree=3, rng_=15.0, vtol=1e-11, seed=3):
    """per level the device's aggregates, T, B_c, lambda, P and A_c against the restatement (from the device's fine A, aggregates and
    lambda), then one V-cycle.  The input condition comes first: no link of any level nearer to the threshold than MARGIN.
    -> (levels, per-level records of _np_aggregate, the largest deviations)"""
    import torch

    assert amg.num_levels >= 2
    levels = ar._restate(amg, B0)
    infos, dev = [], {"T": 0.0, "Bc": 0.0, "lambda": 0.0, "P": 0.0, "Ac": 0.0}
    for l, (A, P, T, B, Bc, agg, lam) in enumerate(levels[:-1]):
        b, nb = amg.level_info(l)["block_size"], B.shape[1]
        info = {}
        agg_np, _ = ar._np_aggregate(A, b, theta, info)
        info["dropped"] = int((Bc.reshape(-1, nb, nb)[:, np.arange(nb), np.arange(nb)] == 0).sum())
        infos.append(info)
        assert info["margin"] >= MARGIN, (l, info)
        assert np.array_equal(agg, agg_np), l
        Td, Bcd = amg.level_matrix(l, "T"), amg.level_matrix(l + 1, "B").toarray()
        dev["T"] = max(dev["T"], _rel(Td, T))
        dev["Bc"] = max(dev["Bc"], np.abs(Bcd - Bc).max() / max(1.0, np.abs(Bc).max()))
        dev["lambda"] = max(dev["lambda"], abs(lam - ar._np_lambda(A, b, agg < 0, steps)) / lam)
        dev["P"] = max(dev["P"], _rel(amg.level_matrix(l, "P"), P))
        Ac_dev = amg.level_matrix(l + 1, "A")
        dev["Ac"] = max(dev["Ac"], _rel(Ac_dev, levels[l + 1][0]))
        print("level", l, "dofs", A.shape[0], info, {k: float(v) for k, v in dev.items()})
        assert dev["T"] <= 1e-12 and dev["Bc"] <= 1e-12 and dev["lambda"] <= 1e-8 and dev["P"] <= 1e-12 and dev["Ac"] <= 1e-12, (l, dev)
        assert (Ac_dev != Ac_dev.T).nnz == 0
    r = np.random.default_rng(seed).standard_normal(levels[0][0].shape[0])
    z = torch.zeros(len(r), dtype=torch.float64, device="cuda")
    amg.apply(torch.from_numpy(r).cuda(), z)
    zn = ar._np_vcycle(levels, r, 0, degree, rng_)
    dev["vcycle"] = float(np.linalg.norm(z.cpu().numpy() - zn) / np.linalg.norm(zn))
    print("levels", [lv[0].shape[0] for lv in levels], "V-cycle", dev["vcycle"], "tolerance", vtol)
    assert dev["vcycle"] <= vtol, dev
    return levels, infos, dev


def _pcg(engine, csr, b, levels=None, **smoother):
    """(the device's AMG-PCG count to 1e-8 with the attached hierarchy, the restatement's when levels are given); the residual as
    test_amg.py::_iters checks it"""
    import torch

    u = torch.zeros_like(b)
    it = engine.cg_solve(csr.values, b, u, fa.PRECOND_AMG, 1e-8)
    res = engine_spmv_residual(engine, csr, u, b)
    assert res <= 1e-7, res
    npc = ar._np_pcg(levels, b.cpu().numpy(), **smoother) if levels is not None else None
    print("AMG-PCG: device", it, "numpy", npc, "residual", res)
    if npc is not None:
        assert abs(it - npc) <= 2, (it, npc)
    return it, u


def _stretched(name, k, axis, stretch, power):
    """the uniform mesh with coordinate `axis` mapped to stretch x^power.  (On a uniformly stretched Quad4 mesh the diagonal link of a free
    corner sits at exactly 0.25 sqrt(||A_ii|| ||A_jj||) whatever the stretch; the mild grading moves it off the threshold.)"""
    m = _mesh(name, k)
    v = m.vertices.copy()
    v[:, axis] = stretch * v[:, axis] ** power
    return fa.Mesh(v, m.connectivity, m.elem_kind)


# (mesh, k, stretched axis, stretch, grading power, theta, NumPy PCG too).  The last one has three levels: the filter on a coarse level
STRENGTH_CASES = [("quad4", 64, 1, 0.6, 1.05, 0.1, True), ("quad4", 64, 1, 0.1, 1.05, 0.25, True), ("hex8", 16, 2, 0.1, 1.0, 0.25, True),
                  ("quad4", 128, 1, 0.1, 1.05, 0.25, False)]


def _oracle_system(o, m, op):
    """the CPU oracle's assembled matrix with the clamp at x = 0 applied as _system applies it on the device: (A, clamped nodes, s)"""
    w, pts = RULES[m.elem_kind]()
    params = None if op == "laplace" else fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.3)).as_pair()
    asm = o.ElementAssembler({fa.HEX8: o.HEX8, fa.QUAD4: o.QUAD4}[m.elem_kind], o.LAPLACE if op == "laplace" else o.LINEAR_ELASTIC, m.vertices,
                             m.connectivity, w, pts, params=params)
    st, _, ro, ci, v = o.assemble(asm)
    assert st == 0
    s = 1 if op == "laplace" else m.vertices.shape[1]
    x0 = m.vertices[:, 0]
    clamp = np.where(x0 <= x0.min() + 1e-9 * (x0.max() - x0.min()))[0]
    o.apply_homogeneous_dirichlet_bc_csr(ro, ci, v, clamp, s)
    return sp.csr_matrix((v, ci.astype(np.int64), ro.astype(np.int64))), clamp, s


@pytest.mark.parametrize("name,k,axis,stretch,power,theta,with_pcg", STRENGTH_CASES)
def test_strength_cases_keep_off_the_threshold(oracle, name, k, axis, stretch, power, theta, with_pcg):
    """the input conditions of test_strength_threshold_scalar hold for the restatement alone: every link of every level at least MARGIN
    from the threshold, weak links on every level, and (the last case) three levels"""
    m = _stretched(name, k, axis, stretch, power)
    A, clamp, s = _oracle_system(oracle, m, "laplace")
    info = []
    levels = ar._restate(None, np.ones((A.shape[0], 1)), A0=A, b0=s, theta=theta, info=info)
    print([lv[0].shape[0] for lv in levels], info)
    assert len(levels) >= (2 if with_pcg else 3)
    assert all(i["margin"] >= MARGIN and 0 < i["weak"] and 0 < i["strong"] for i in info)
    weak = [i["weak"] / (i["weak"] + i["strong"]) for i in info]
    assert len(set(weak)) == len(weak)
    # a uniform stretch cannot do that on Quad4: the free corners' diagonal links are at 0.25, to rounding
    if name == "quad4" and theta == 0.25:
        mu = _mesh(name, k)
        mu.vertices[:, axis] *= stretch
        assert ar._strength(_oracle_system(oracle, mu, "laplace")[0], 1, theta)[2] < 1e-12


def test_weakened_nodes_become_one_node_aggregates(oracle):
    """the input conditions of test_strength_threshold_blocks_one_node_aggregates for the restatement alone; and D A D alone would not do:
    the strength measure is invariant under it"""
    m = _mesh("hex8", 12)
    A, clamp, s = _oracle_system(oracle, m, "elastic")
    nodes = _spread_nodes(ar._node_graph(A, s), _interior(m), 27, 7)
    d = np.ones(A.shape[0])
    d[(s * nodes[:, None] + np.arange(s)).ravel()] = 1e-3
    S0, S1 = ar._strength(A, s, 0.05)[0], ar._strength((sp.diags(d) @ A @ sp.diags(d)).tocsr(), s, 0.05)[0]
    assert (S0 != S1).nnz == 0
    info = {}
    agg, _ = ar._np_aggregate(_weaken(A, s, nodes, 1e-3), s, 0.05, info)
    print(info)
    assert info["margin"] >= MARGIN and info["one_node"] == 27 >= 20 and 0 < info["weak"] < info["strong"]
    assert (np.bincount(agg[agg >= 0])[agg[nodes]] == 1).all()
    assert 6 * (agg.max() + 1) <= 0.9 * A.shape[0]   # (the create is not refused)


def test_box_and_one_element_has_three_levels(oracle):
    """the input condition of test_isolated_node_on_a_coarse_level: ISO_COARSE_K is the smallest k whose first coarse level has more than
    4096 dofs, and the extra element's free nodes are one aggregate"""
    for k, three in ((ISO_COARSE_K - 1, False), (ISO_COARSE_K, True)):
        m, extra = _box_and_one_element(k)
        A, clamp, s = _oracle_system(oracle, m, "elastic")
        agg, _ = ar._np_aggregate(A, s)
        assert (6 * (agg.max() + 1) > 4096) == three, (k, agg.max() + 1)
    free = np.setdiff1d(extra, clamp)
    assert len(free) == 4 and np.array_equal(np.where(agg == agg[free[0]])[0], free)


@pytest.mark.gpu
@pytest.mark.parametrize("name,k,axis,stretch,power,theta,with_pcg", STRENGTH_CASES)
def test_strength_threshold_scalar(engine, name, k, axis, stretch, power, theta, with_pcg):
    m = _stretched(name, k, axis, stretch, power)
    asm, csr, clamp, s = _system(engine, m, "laplace")
    b = _rhs(m.num_nodes(), s, clamp)
    B0 = np.ones((m.num_nodes(), 1))
    it0 = None
    if with_pcg:
        amg0 = fa.SmoothedAggregationAMG(asm, csr, near_nullspace="constant")
        it0, _ = _pcg(engine, csr, b)
        amg0.close()
    amg = fa.SmoothedAggregationAMG(asm, csr, near_nullspace="constant", theta=theta)
    levels, infos, dev = _parity(amg, B0, theta)
    # the case tests something: weak links on every coarsened level, another share of them from one level to the next
    weak = [i["weak"] / (i["weak"] + i["strong"]) for i in infos]
    assert all(0 < w < 1 for w in weak) and len(set(weak)) == len(weak), weak
    if not with_pcg:
        assert amg.num_levels >= 3
    else:
        it, _ = _pcg(engine, csr, b, levels)
        print("theta", theta, "iterations", it, "theta 0", it0)
        assert it <= it0, (it, it0)   # the filter pays for itself on the mesh it is meant for
    amg.close()


def _interior(m):
    x = m.vertices
    return np.where(((x > 1e-9) & (x < 1 - 1e-9)).all(axis=1))[0]


@pytest.mark.gpu
def test_strength_threshold_blocks_one_node_aggregates(engine):
    """Hex8 elasticity with 27 (2 %) of the interior nodes, pairwise non-adjacent, weakened: D A D with D = 1e-3 on their dofs and their
    diagonal blocks put back (_weaken: SPD, on the pattern).  At theta = 0.05 they keep nonzero blocks but no strong link, so each is an
    aggregate of its own, with 3 rows for 6 rigid-body modes: the three rotations are dropped, and the coarse matrix has zero rows,
    columns and diagonal entries there"""
    import torch

    theta = 0.05
    m = _mesh("hex8", 12)
    asm, csr, clamp, s = _system(engine, m, "elastic")
    G = ar._node_graph(csr.to_scipy(), s)
    nodes = _spread_nodes(G, _interior(m), 27, 7)

    def edit(v, rn, cn, ra, ca):
        v[np.isin(rn, nodes) ^ np.isin(cn, nodes)] *= 1e-3

    _values_on_pattern(csr, s, edit)
    amg = fa.SmoothedAggregationAMG(asm, csr, near_nullspace="rigid_body", theta=theta)
    levels, infos, dev = _parity(amg, ar._rigid(m), theta)
    assert infos[0]["one_node"] >= 20 and 0 < infos[0]["weak"] < infos[0]["strong"], infos[0]
    agg = amg.aggregates(0)
    single = np.where(np.bincount(agg[agg >= 0]) == 1)[0]
    assert np.array_equal(np.sort(agg[nodes]), single)   # the weakened nodes, and only they
    Td, A1 = amg.level_matrix(0, "T").tocsc(), amg.level_matrix(1, "A")
    A1c = A1.tocsc()
    for i in nodes:
        cols = 6 * agg[i] + np.arange(6)
        live = np.array([abs(Td[:, c]).sum() > 0 for c in cols])
        assert live.sum() == 3 and np.array_equal(Td[3 * i:3 * i + 3][:, cols[live]].toarray(), np.eye(3))
        dead = cols[~live]
        assert not A1[dead].data.any() and not A1c[:, dead].data.any()
    assert infos[0]["dropped"] == 3 * len(nodes)
    assert (A1 != A1.T).nnz == 0
    n = s * m.num_nodes()
    g = torch.Generator(device="cpu").manual_seed(0)
    x, y = (torch.randn(n, generator=g, dtype=torch.float64).cuda() for _ in range(2))
    Bx, By, Bx2 = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    amg.apply(x, Bx)
    amg.apply(y, By)
    amg.apply(x, Bx2)
    p, q = float(x @ By), float(y @ Bx)
    print("x.By - y.Bx", abs(p - q) / max(abs(p), abs(q)), "one-node aggregates", len(single), "dropped", infos[0]["dropped"])
    assert abs(p - q) <= 1e-12 * max(abs(p), abs(q))
    assert float(x @ Bx) > 0 and float(y @ By) > 0
    assert torch.equal(Bx, Bx2)
    _pcg(engine, csr, _rhs(n, s, clamp), levels)
    amg.close()


@pytest.mark.gpu
def test_dependent_near_nullspace_column_is_dropped(engine):
    """nb = 6 on s = 1: constant, x, y, z, xy and an exact copy of x.  The copy is dropped in every aggregate, by the relative rule (what
    Gram-Schmidt leaves of it is rounding noise, not zero)"""
    m = _mesh("hex8", 17)
    asm, csr, clamp, s = _system(engine, m, "laplace")
    x = m.vertices
    B0 = np.stack([np.ones(len(x)), x[:, 0], x[:, 1], x[:, 2], x[:, 0] * x[:, 1], x[:, 0]], axis=1)
    amg = fa.SmoothedAggregationAMG(asm, csr, near_nullspace=B0)
    levels, infos, dev = _parity(amg, B0)
    nagg = amg.aggregates(0).max() + 1
    Td, A1 = amg.level_matrix(0, "T").tocsc(), amg.level_matrix(1, "A")
    Rm = amg.level_matrix(1, "B").toarray().reshape(nagg, 6, 6)
    copy = 6 * np.arange(nagg) + 5
    assert not Rm[:, 5, :].any() and abs(Td[:, copy]).sum() == 0
    assert (Rm[:, np.arange(5), np.arange(5)] > 0).all()   # the five independent columns stay
    assert np.allclose(Rm[:, :2, 5], Rm[:, :2, 1], rtol=1e-12, atol=0)   # (the copy's projections: T B_c = B holds for it too)
    assert not A1[copy].data.any() and not A1.tocsc()[:, copy].data.any()
    assert infos[0]["dropped"] == nagg
    print("aggregates", nagg, "dropped", infos[0]["dropped"])
    _pcg(engine, csr, _rhs(m.num_nodes(), s, clamp), levels)
    amg.close()


@pytest.mark.gpu
def test_isolated_nodes_with_real_blocks(engine):
    """30 interior nodes cut out of a clamped Hex8 elasticity matrix (their off-diagonal blocks zero: a direct sum, so SPD); 5 of them get
    the rank-2 block v v^T + w w^T of small integers, whose third pivot is exactly zero, so that dof is left out"""
    import torch

    m = _mesh("hex8", 12)
    asm, csr, clamp, s = _system(engine, m, "elastic")
    rng = np.random.default_rng(19)
    nodes = np.sort(rng.choice(_interior(m), 30, replace=False))
    deficient = nodes[::6]
    assert len(deficient) == 5
    v, w = np.array([2.0, 1.0, 2.0]), np.array([0.0, 3.0, 3.0])
    M = 2.0 ** 16 * (np.outer(v, v) + np.outer(w, w))

    def edit(val, rn, cn, ra, ca):
        val[(np.isin(rn, nodes) | np.isin(cn, nodes)) & (rn != cn)] = 0.0
        own = np.isin(rn, deficient) & (rn == cn)
        val[own] = M[ra[own], ca[own]]

    _values_on_pattern(csr, s, edit)
    amg = fa.SmoothedAggregationAMG(asm, csr, near_nullspace="rigid_body")
    agg = amg.aggregates(0)
    iso = np.union1d(nodes, clamp.astype(np.int64))
    assert np.array_equal(np.where(agg < 0)[0], iso) and (agg[agg < 0] == -1).all()
    P = amg.level_matrix(0, "P")
    dofs = (s * iso[:, None] + np.arange(s)).ravel()
    assert abs(P[dofs]).sum() == 0
    # the V-cycle's tolerance: 1e-11, or 50 cond eps of the worst kept block
    A = amg.level_matrix(0, "A")
    cond = 1.0
    for i, Mi in zip(iso, ar._diagonal_blocks(A, iso, s)):
        out = ar._iso_inverse(Mi)[1]
        assert out.any() == (i in deficient) and (not out.any() or np.array_equal(out, [False, False, True])), (i, out)
        cond = max(cond, np.linalg.cond(Mi[np.ix_(~out, ~out)]))
    vtol = max(1e-11, 50 * cond * EPS)
    print("largest cond of a kept block", cond, "V-cycle tolerance", vtol, "(the 1e-11 of the parity test)" if vtol == 1e-11 else "(50 cond eps)")
    levels, infos, dev = _parity(amg, ar._rigid(m), vtol=vtol)
    # the dof left out gets exactly zero, whatever the right-hand side holds there
    n = s * m.num_nodes()
    r = torch.from_numpy(np.random.default_rng(3).standard_normal(n)).cuda()
    z = torch.zeros_like(r)
    amg.apply(r, z)
    assert (z.cpu().numpy()[s * deficient + 2] == 0).all() and (z.cpu().numpy()[s * deficient] != 0).all()
    _pcg(engine, csr, _rhs(n, s, np.union1d(clamp.astype(np.int64), deficient)), levels)
    amg.close()


def _box_and_one_element(k):
    """the unit box of k^3 elements and one more element of the same size beside it (shifted by 2 in y, its x = 0 face under the same
    clamp), as one mesh; (mesh, the nodes of the extra element)"""
    m = _mesh("hex8", k)
    v0 = m.vertices[m.connectivity[0].astype(np.int64)]
    extra = v0 - v0.min(axis=0) + np.array([0.0, 2.0, 0.0])
    n = m.num_nodes()
    conn = np.concatenate([m.connectivity, (n + np.arange(8)).astype(m.connectivity.dtype)[None, :]])
    return fa.Mesh(np.concatenate([m.vertices, extra]), conn, m.elem_kind), n + np.arange(8)


ISO_COARSE_K = 30   # the smallest k with three levels: 694 aggregates, 4164 coarse dofs (k = 29: 612 aggregates, 3672 dofs, two levels)


@pytest.mark.gpu
def test_isolated_node_on_a_coarse_level(engine):
    """The extra element's 4 free nodes are one aggregate, a coarse node with an SPD 6 x 6 diagonal block and no other: isolated on level
    1, inverted by the Cholesky kernel at its largest block size.  The restatement takes seconds at this size, so levels 0 and 1 and the
    V-cycle are compared; the NumPy PCG is left out (the device's PCG has to converge)"""
    m, extra = _box_and_one_element(ISO_COARSE_K)
    asm, csr, clamp, s = _system(engine, m, "elastic")
    amg = fa.SmoothedAggregationAMG(asm, csr, near_nullspace="rigid_body")
    assert amg.num_levels >= 3
    free = np.setdiff1d(extra, clamp.astype(np.int64))
    assert len(free) == 4
    agg0, agg1 = amg.aggregates(0), amg.aggregates(1)
    J = agg0[free[0]]
    assert J >= 0 and np.array_equal(np.where(agg0 == J)[0], free)
    assert np.array_equal(np.where(agg1 < 0)[0], [J])
    A1 = amg.level_matrix(1, "A")
    blk = A1[6 * J:6 * J + 6].tocoo()
    assert (blk.col[blk.data != 0] // 6 == J).all() and not A1.tocsc()[:, 6 * J:6 * J + 6][np.r_[0:6 * J, 6 * J + 6:A1.shape[0]]].data.any()
    D = A1[6 * J:6 * J + 6][:, 6 * J:6 * J + 6].toarray()
    assert np.linalg.eigvalsh(D).min() > 0 and not ar._iso_inverse(D)[1].any()
    assert abs(amg.level_matrix(1, "P")[6 * J:6 * J + 6]).sum() == 0
    levels, infos, dev = _parity(amg, ar._rigid(m))
    assert len(levels) >= 3
    _pcg(engine, csr, _rhs(s * m.num_nodes(), s, clamp))
    amg.close()


def _snapshot(amg, r):
    import torch

    z = torch.zeros_like(r)
    amg.apply(r, z)
    mats = [amg.level_matrix(l, "A").data for l in range(1, amg.num_levels)] + [amg.level_matrix(l, "P").data for l in range(amg.num_levels - 1)]
    return mats, [amg.level_info(l)["lambda_max"] for l in range(amg.num_levels)], z.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("degree,rng_,steps", [(1, 4.0, 5), (5, 30.0, 20)])
@pytest.mark.parametrize("name,k,op,ns", [("hex8", 17, "laplace", "constant"), ("quad4", 52, "elastic", "rigid_body")])
def test_smoother_parameters(engine, name, k, op, ns, degree, rng_, steps):
    """lambda follows eig_steps, P and A_c the new lambda, the V-cycle degree and range; the constructor and fh_amg_set_smoother on a
    default hierarchy give the same bits"""
    import torch

    m = _mesh(name, k)
    asm, csr, clamp, s = _system(engine, m, op)
    B0 = ar._rigid(m) if ns == "rigid_body" else np.kron(np.ones((m.num_nodes(), 1)), np.eye(s))
    r = torch.from_numpy(np.random.default_rng(3).standard_normal(s * m.num_nodes())).cuda()
    amg = fa.SmoothedAggregationAMG(asm, csr, near_nullspace=ns, degree=degree, smoothing_range=rng_, eig_steps=steps)
    _parity(amg, B0, steps=steps, degree=degree, rng_=rng_)
    one = _snapshot(amg, r)
    amg.close()
    amg = fa.SmoothedAggregationAMG(asm, csr, near_nullspace=ns)
    default = _snapshot(amg, r)
    assert _ffi.lib().fh_amg_set_smoother(amg._h, degree, rng_, steps) == 0
    two = _snapshot(amg, r)
    amg.close()
    assert one[1] == two[1] and all(np.array_equal(p, q) for p, q in zip(one[0], two[0])) and np.array_equal(one[2], two[2])
    # and they are not the default's: every parameter reaches the device
    assert default[1][0] != one[1][0] and not np.array_equal(default[0][-1], one[0][-1]) and not np.array_equal(default[2], one[2])


@pytest.mark.gpu
def test_refusals_leave_the_context_usable(engine):
    import torch

    lib = _ffi.lib()
    m = _mesh("quad4", 72)
    asm, csr, clamp, s = _system(engine, m, "laplace")
    vp = C.c_void_p(csr.values.data_ptr())
    # theta = 10: nothing is strong, every node is an aggregate of its own, and the step keeps more than 90 % of the dofs
    for theta, code in ((10.0, FH_UNSUPPORTED), (-1.0, FH_BAD_ARGUMENT), (float("nan"), FH_BAD_ARGUMENT)):
        h = C.c_void_p(12345)
        assert lib.fh_amg_create(engine._h, vp, _ffi.AMG_CONSTANT, None, 0, theta, 0, C.byref(h)) == code, theta
        assert not h.value   # (no handle: the output is null)
    with pytest.raises(_ffi.FenrisError) as e:
        fa.SmoothedAggregationAMG(asm, csr, near_nullspace="constant", theta=10.0)
    assert e.value.code == FH_UNSUPPORTED
    b = _rhs(m.num_nodes(), s, clamp)
    amg = fa.SmoothedAggregationAMG(asm, csr, near_nullspace="constant")
    fresh_engine = fa.Engine(0)
    asm2, csr2, _, _ = _system(fresh_engine, m, "laplace")
    fresh = fa.SmoothedAggregationAMG(asm2, csr2, near_nullspace="constant")
    assert amg.num_levels == fresh.num_levels >= 2
    for l in range(amg.num_levels - 1):
        assert np.array_equal(amg.aggregates(l), fresh.aggregates(l))
        assert np.array_equal(amg.level_matrix(l, "P").data, fresh.level_matrix(l, "P").data)
        assert np.array_equal(amg.level_matrix(l + 1, "A").data, fresh.level_matrix(l + 1, "A").data)
    it, u = _pcg(engine, csr, b)
    it2, u2 = _pcg(fresh_engine, csr2, b)
    assert it == it2 and torch.equal(u, u2)
    fresh.close()
    amg.close()
    fresh_engine.close()


@pytest.mark.gpu
def test_numeric_refresh_under_theta(engine):
    """values scaled by 2 (exact in binary floating point): the aggregates are kept, lambda of D^-1 A and P keep their bits (lambda and D
    scale together), A_c doubles"""
    name, k, axis, stretch, power, theta, _ = STRENGTH_CASES[1]
    m = _stretched(name, k, axis, stretch, power)
    asm, csr, clamp, s = _system(engine, m, "laplace")
    amg = fa.SmoothedAggregationAMG(asm, csr, near_nullspace="constant", theta=theta)
    assert amg.num_levels >= 2
    before = [(amg.aggregates(l), amg.level_matrix(l, "P"), amg.level_matrix(l + 1, "A")) for l in range(amg.num_levels - 1)]
    info = {}
    ar._np_aggregate(amg.level_matrix(0, "A"), s, theta, info)
    assert info["weak"] > 0 and info["margin"] >= MARGIN
    amg.update(type(csr)(csr.row_offsets, csr.col_indices, 2.0 * csr.values))
    for l, (agg, P, Ac) in enumerate(before):
        assert np.array_equal(amg.aggregates(l), agg)
        assert np.array_equal(amg.level_matrix(l, "P").data, P.data)
        Ac2 = amg.level_matrix(l + 1, "A")
        print("level", l + 1, "|A_c(2 A) - 2 A_c| / |2 A_c|", _rel(Ac2, 2.0 * Ac))
        assert _rel(Ac2, 2.0 * Ac) <= 1e-14
    amg.close()
