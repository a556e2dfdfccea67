"""The kernels that walk the node-blocked CSR -- SpMV (half a wavefront or a wavefront per node), the x . y partials and their range sums,
the CG vector kernels, the Jacobi diagonal, the Dirichlet rows and right-hand side -- on crafted patterns with values the test supplies:
no finite element assembly in between.  Patterns are cut to the lane, trip and range boundaries of the kernels (csr_reference.py); values
are non-symmetric and, where the check is bitwise, integers or dyadic numbers small enough that every sum is exact in any order.

CPU part: the generators against inc^T inc, the layout against its definition, the long-double reference against fractions.Fraction, and the
exactness budgets of every bitwise case.  GPU part: sections 1-5 below, all on one Engine."""
import contextlib
import functools
import zlib
from fractions import Fraction

import numpy as np
import pytest

import fenris_amd as fa
import csr_reference as cr

SDIMS = [1, 2, 3]
WAVE_OPTION = "FENRIS_HIP_SPMV_WAVE_PER_NODE"
HALF, FULL = "k_spmv_blocked_half", "k_spmv_blocked"

# ---- the patterns
HALF_STARS = [2, 16, 17, 31, 32]            # max_row <= 32: half a wavefront per node by default, lanes 0 / 15 / 16 / 30 / 31 the last active
FULL_STARS = [33, 63, 64, 65, 130, 700]     # a wavefront per node: S * k entries around the trips of 64, and many trips
PAD_NODES = [1, 2, 3, 15, 16, 17, 33]       # tails of the 16-node and of the 4-node workgroup
PATTERNS, INTENDED = {}, {}               # name -> Pattern, name -> (nodes, blocks of the longest row) as the case means them


def _add(p, num_nodes, max_row, name=None):
    PATTERNS[name or p.name] = p
    INTENDED[name or p.name] = (num_nodes, max_row)
    return name or p.name


SMALL = ([_add(cr.star(k), k, k) for k in HALF_STARS + FULL_STARS] + [_add(cr.clique(k), k, k) for k in (32, 33)]
         # a row of one block and a row of none behind a star of either kernel
         + [_add(cr.with_isolated(cr.with_single(cr.star(k))), k + 2, k) for k in (17, 40)]
         + [_add(cr.padded(n), n, min(n, 9)) for n in PAD_NODES])
# the range sums: more per-workgroup partials than the 2048 ranges of the SpMV (2050 for either kernel), and more than the 1024 of the vector kernels
LONG = [_add(cr.with_chain(cr.star(40), 8197), 8197, 40, "full8197"), _add(cr.with_chain(cr.star(2), 32785), 32785, 3, "half32785"),
        _add(cr.with_chain(cr.star(2), 90001), 90001, 3, "vec90001")]
# full solves: a few hundred nodes around one long row
SOLVES = [_add(cr.with_chain(cr.star(65), 300), 300, 65, "solve65"), _add(cr.with_chain(cr.star(32), 301), 301, 32, "solve32")]

CG_STEP = ["star32", "star33", "star65"] + LONG
ROUNDING = ["star32", "star65", "star700"]
DIRICHLET = ["star16", "star32", "star33", "star64", "star65", "star130", "star17+single+isolated"]


def _seed(*key):
    """a generator per case, the same in every run and whatever the order of the tests"""
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


@functools.lru_cache(maxsize=None)
def _host(name, S):
    """the expected pattern of PATTERNS[name] with S components, from the incidence matrix"""
    p = PATTERNS[name]
    noff, ncols = cr.node_pattern(p)
    ro, ci = cr.scalar_pattern(noff, ncols, S)
    return {"p": p, "noff": noff, "ncols": ncols, "ro": ro, "ci": ci, "n": S * p.num_nodes}


@functools.lru_cache(maxsize=None)
def _cg_step_system(name, S, jacobi):
    """(values, b, x1, budget) of section 3: left unchanged by the tests that share it"""
    h = _host(name, S)
    rng = _seed("cg", name, S, jacobi)
    values, e = cr.dominant_integer_values(rng, h["ro"], h["ci"], jacobi)
    b = cr.integer_values(rng, h["n"], 1 << 8)
    x1, budget = cr.cg_first_step(h["ro"], h["ci"], values, b, e)
    for a in (values, b) + ((x1,) if x1 is not None else ()):
        a.setflags(write=False)
    return values, b, x1, budget


# =================================================================================================================== CPU
@pytest.mark.parametrize("name", list(PATTERNS))
def test_generators_produce_the_intended_rows(name):
    """the row lengths each generator states, and the sizes each case is meant to have, against the pattern of inc^T inc"""
    p = PATTERNS[name]
    noff, ncols = cr.node_pattern(p)
    cnt = np.diff(noff)
    assert np.array_equal(cnt, p.counts)
    assert (len(cnt), int(cnt.max())) == INTENDED[name] == (p.num_nodes, p.max_row)
    rows = cr.row_of_entry(noff)
    assert np.all((np.diff(ncols) > 0) | (np.diff(rows) > 0))                  # ascending inside every row
    assert np.all(ncols[cr.diagonal_positions(noff, ncols)[cnt > 0]] == np.nonzero(cnt > 0)[0])
    if name.startswith("star") and name[4:].isdigit():
        assert cnt[0] == len(cnt) and np.all(cnt[1:] == 2)
    if "+single+isolated" in name:
        assert list(cnt[-2:]) == [1, 0]


def test_kernel_boundaries_are_the_ones_the_patterns_aim_at():
    """the launch arithmetic of spmv_launch / fh_cg_solve_dev / cg_run, restated: which cases have more partials than ranges and ranges of
    more than one partial"""
    grid = lambda n, half: (n + 15) // 16 if half else (n + 3) // 4
    gs = lambda n: min(2048, (n + 3) // 4)
    per = lambda count, ranges: -(-count // ranges)
    assert grid(8197, False) == 2050 and gs(8197) == 2048 and per(2050, 2048) == 2
    assert grid(32785, True) == 2050 and gs(32785) == 2048 and per(2050, 2048) == 2
    assert per(grid(32785, False), gs(32785)) == 5 and per(grid(90001, True), gs(90001)) == 3
    n = 3 * 90001
    assert n > 262144 and per((n + 255) // 256, min(1024, (n + 255) // 256)) == 2
    for name in SMALL + SOLVES:                          # the small cases: fewer partials than ranges, most ranges empty
        N = PATTERNS[name].num_nodes
        assert grid(N, True) <= gs(N) and grid(N, False) == gs(N)
    assert {PATTERNS[f"star{k}"].max_row for k in HALF_STARS} == set(HALF_STARS) and max(HALF_STARS) == 32 < min(FULL_STARS)
    assert [S * k for S in SDIMS for k in (63, 64, 65)] == [63, 64, 65, 126, 128, 130, 189, 192, 195]   # entries of the hub row around the trips


@pytest.mark.parametrize("S", SDIMS)
def test_scalar_layout_matches_its_definition(S):
    for p in (cr.star(5), cr.clique(4), PATTERNS["star17+single+isolated"], PATTERNS["single"]):
        noff, ncols = cr.node_pattern(p)
        ro, ci = cr.scalar_pattern(noff, ncols, S)
        ro2, ci2 = cr.scalar_pattern_naive(noff, ncols, S)
        assert np.array_equal(ro, ro2) and np.array_equal(ci, ci2)
        dpos = cr.diagonal_positions(ro, ci)
        for r in range(len(ro) - 1):
            has = p.counts[r // S] > 0
            assert (dpos[r] >= 0) == has and (not has or (ci[dpos[r]] == r and ro[r] <= dpos[r] < ro[r + 1]))


def _need_longdouble():
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip("np.longdouble has no 64-bit mantissa on this platform")


def _exact(v):
    """a long double with a 64-bit mantissa as a Fraction: the sum of two doubles"""
    hi = np.float64(v)
    return Fraction(float(hi)) + Fraction(float(np.float64(v - hi)))


def test_longdouble_reference_agrees_with_fractions():
    _need_longdouble()
    p = cr.with_isolated(cr.star(6))
    noff, ncols = cr.node_pattern(p)
    ro, ci = cr.scalar_pattern(noff, ncols, 2)
    rng = _seed("fraction")
    values, x = cr.scaled_normals(rng, len(ci)), cr.scaled_normals(rng, len(ro) - 1)
    y, ay = cr.spmv_longdouble(ro, ci, values, x)
    yf, ayf = cr.spmv_fraction(ro, ci, values, x)
    assert any(v != 0 for v in yf)
    for r in range(len(ro) - 1):
        n = int(ro[r + 1] - ro[r])
        # n products and n - 1 additions, each rounded to 64 bits: far inside the 2^-53 (|A||x|)_i the device bound grants the reference
        assert abs(_exact(y[r]) - yf[r]) <= n * Fraction(1, 1 << 64) * ayf[r] * Fraction(101, 100)
        assert abs(_exact(ay[r]) - ayf[r]) <= n * Fraction(1, 1 << 64) * ayf[r] * Fraction(101, 100)
    assert ro[-1] == ro[-3] and y[-1] == 0 and ay[-1] == 0 and yf[-1] == 0        # the rows of no blocks


def test_integer_spmv_budget():
    """|a| <= 2^10, |x| <= 2^8, at most 3 * 700 entries per row: every partial sum stays below 2^30, far below 2^53"""
    assert (1 << 10) * (1 << 8) * 3 * max(PATTERNS[n].max_row for n in PATTERNS) < (1 << 30) < cr.EXACT
    h = _host("star700", 3)
    rng = _seed("spmv", "star700", 3)
    values, x = cr.integer_values(rng, len(h["ci"]), 1 << 10), cr.integer_values(rng, h["n"], 1 << 8)
    assert np.abs(values).max() == 1 << 10 and np.abs(x).max() <= 1 << 8
    _, bound = cr.spmv_int(h["ro"], h["ci"], values, x)
    assert bound < 1 << 30


@pytest.mark.parametrize("jacobi", [False, True], ids=["identity", "jacobi"])
@pytest.mark.parametrize("S", SDIMS)
@pytest.mark.parametrize("name", CG_STEP)
def test_cg_step_exactness_budget(name, S, jacobi):
    """Bit budget of section 3, in units of 2^-E (z . r), 2^-2E (p . A p) with E the largest exponent of the diagonal (E = 0 for the identity).
    |b| <= 2^8.  Jacobi: z = 2^-e b with e spanning DIAG_SPAN + 1 = 4 values, so the integers Z = 2^E z have |Z| <= 2^11; the diagonal is at
    most 2^(e0 + 3) with 2^e0 just above the largest absolute off-diagonal sum (3 (3 * 65 - 1) < 2^10 for the star of 65 with S = 3, 24 < 2^5
    on a chain), so (|A||Z|)_i <= 2 * 2^13 * 2^11 = 2^25 in a star's rows and 2^20 in a chain's, and sum_i |Z_i| (|A||Z|)_i over the 270003 <
    2^19 rows of the longest chain is below 2^(19 + 11 + 20) = 2^50.  cg_first_step forms the actual sums of absolute values in integers (the
    largest is 2^43, Jacobi on the two longest chains with S = 3): they bound every partial sum in any order and have to stay below 2^53."""
    values, b, x1, budget = _cg_step_system(name, S, jacobi)
    h = _host(name, S)
    assert budget < cr.EXACT and x1 is not None, budget
    assert np.array_equal(values, np.rint(values)) and np.abs(b).max() <= 1 << 8
    a = cr.to_scipy(h["ro"], h["ci"], values)
    assert (a != a.T).nnz > 0                                                   # not symmetric
    d = a.diagonal()
    rows, cols = np.asarray(abs(a).sum(axis=1)).ravel() - np.abs(d), np.asarray(abs(a).sum(axis=0)).ravel() - np.abs(d)
    assert np.all(d > rows) and np.all(d > cols)
    if jacobi:
        m, e = np.frexp(d)
        assert np.all(m == 0.5) and len(set(e)) == min(cr.DIAG_SPAN + 1, len(d))
        if S > 1:
            assert all(len(set(e[S * i:S * i + S])) == S for i in range(PATTERNS[name].num_nodes))


# =================================================================================================================== GPU
@pytest.fixture(scope="module")
def engine():
    eng = fa.Engine(0)
    yield eng
    eng.close()


def _bind(engine, name, S):
    """the pattern on the engine, checked entry for entry: a case cannot silently move to the other kernel"""
    h = _host(name, S)
    p = h["p"]
    fa.MockElementAssembler(S, p.num_nodes, p.elements, engine)
    ro, ci = engine.pattern()
    assert np.array_equal(ro.astype(np.int64), h["ro"]) and np.array_equal(ci.astype(np.int64), h["ci"])
    assert (p.num_nodes, int(np.diff(ro.astype(np.int64))[::S].max())) == (INTENDED[name][0], S * INTENDED[name][1])
    return h


@contextlib.contextmanager
def _kernel(engine, kernel, max_row):
    """run with the SpMV kernel `kernel`: the wavefront-per-node form on a pattern of short rows needs the switch"""
    forced = kernel == FULL and max_row <= 32
    assert kernel == (FULL if max_row > 32 else HALF) or forced
    try:
        if forced:
            engine.set_option(WAVE_OPTION, 1)
        yield
    finally:
        engine.set_option(WAVE_OPTION, None)


def _kernels(max_row):
    return [FULL] if max_row > 32 else [HALF, FULL]


def _spmv(engine, torch, values, x):
    """y = A x into a vector of NaN"""
    y = torch.full((len(x),), float("nan"), dtype=torch.float64, device="cuda:0")
    engine.spmv(torch.from_numpy(values).cuda(), torch.from_numpy(x).cuda(), y)
    return y.cpu().numpy()


# ---- 1. SpMV, bit-exact on integer data
@pytest.mark.gpu
@pytest.mark.parametrize("S", SDIMS)
@pytest.mark.parametrize("name", SMALL + LONG)
def test_spmv_integer_data_is_exact(engine, name, S):
    """independent integers in [-2^10, 2^10] for every entry (no symmetry, neither of the matrix nor of its blocks), x in [-2^8, 2^8]: the
    result is exact whatever the reduction tree, so a misplaced, dropped or transposed entry changes it"""
    import torch

    h = _bind(engine, name, S)
    rng = _seed("spmv", name, S)
    values, x = cr.integer_values(rng, len(h["ci"]), 1 << 10), cr.integer_values(rng, h["n"], 1 << 8)
    ref, bound = cr.spmv_int(h["ro"], h["ci"], values, x)
    assert bound < cr.EXACT
    for kernel in _kernels(h["p"].max_row):
        with _kernel(engine, kernel, h["p"].max_row):
            y = _spmv(engine, torch, values, x)
            assert engine.last_kernel_name() == kernel
        assert not np.isnan(y).any(), (kernel, "rows not written", np.nonzero(np.isnan(y))[0][:8])
        bad = np.nonzero(y != ref)[0]
        assert np.array_equal(y, ref), (kernel, "rows", bad[:8], y[bad[:8]], ref[bad[:8]])


# ---- 2. SpMV, rounding on real data
@pytest.mark.gpu
@pytest.mark.parametrize("S", SDIMS)
@pytest.mark.parametrize("name", ROUNDING)
def test_spmv_real_data_within_the_fma_bound(engine, name, S):
    """|y_i - yhat_i| <= (n_i + 2) 2^-53 (|A||x|)_i, n_i = S cnt_i: n fused multiply-adds summed in any order, the final rounding and the
    error of the long-double reference"""
    import torch

    _need_longdouble()
    h = _bind(engine, name, S)
    rng = _seed("rounding", name, S)
    values, x = cr.scaled_normals(rng, len(h["ci"])), cr.scaled_normals(rng, h["n"])
    ref, absref = cr.spmv_longdouble(h["ro"], h["ci"], values, x)
    bound = (np.diff(h["ro"]) + 2).astype(cr.LD) * cr.LD(2.0) ** -53 * absref
    for kernel in _kernels(h["p"].max_row):
        with _kernel(engine, kernel, h["p"].max_row):
            y = _spmv(engine, torch, values, x)
            assert engine.last_kernel_name() == kernel
        err = np.abs(y.astype(cr.LD) - ref)
        worst = int(np.argmax(err - bound))
        print(f"{name} S={S} {kernel}: max err/bound = {float(np.max(err / bound)):.3g}")
        assert np.all(err <= bound), (kernel, worst, float(err[worst]), float(bound[worst]))


# ---- 3. one CG step, bit-exact
def _one_step(engine, values, b, pre):
    x = np.zeros(len(b))
    try:
        it = engine.cg_solve(values, b, x, pre, rel_tol=1e-300, max_iter=1)
    except fa.CgSolveError as e:
        assert e.kind == "MaxIterationsReached" and e.num_iterations == 1
    else:
        assert it == 1          # (a system this step solves exactly: the residual is zero)
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("jacobi", [False, True], ids=["identity", "jacobi"])
@pytest.mark.parametrize("S", SDIMS)
@pytest.mark.parametrize("name", CG_STEP)
def test_cg_first_step_is_exact(engine, name, S, jacobi):
    """x0 = 0, integer b and A (Jacobi: a power-of-two diagonal): b . b, z . r and p . A p are exact sums (test_cg_step_exactness_budget), so
    x1 = fl(fl(z.r / p.Ap) z) bit for bit -- through the x . y partials of either SpMV kernel, k_sum_partial_ranges with empty ranges and with
    ranges of several partials, k_cg_init, k_cg_update and k_inverse_diagonal"""
    values, b, x1, budget = _cg_step_system(name, S, jacobi)
    assert budget < cr.EXACT
    h = _bind(engine, name, S)
    for kernel in _kernels(h["p"].max_row):
        with _kernel(engine, kernel, h["p"].max_row):
            x = _one_step(engine, values, b, fa.PRECOND_JACOBI if jacobi else fa.PRECOND_IDENTITY)
            assert engine.last_kernel_name() == kernel
        bad = np.nonzero(x != x1)[0]
        assert np.array_equal(x, x1), (kernel, len(bad), bad[:4], x[bad[:4]], x1[bad[:4]])


# ---- 4. full solves off the Hex8 path
@pytest.mark.gpu
@pytest.mark.parametrize("jacobi", [False, True], ids=["identity", "jacobi"])
@pytest.mark.parametrize("S", SDIMS)
@pytest.mark.parametrize("name", SOLVES)
def test_cg_solves_match_oracle(engine, oracle, name, S, jacobi):
    tol = 1e-10
    h = _bind(engine, name, S)
    rng = _seed("solve", name, S)
    values = cr.symmetric_dominant_values(rng, h["ro"], h["ci"])
    b = rng.standard_normal(h["n"])
    a = cr.to_scipy(h["ro"], h["ci"], values)
    st, x_ref, it_ref = oracle.cg_solve(h["ro"], h["ci"], values, b, jacobi=jacobi, tol=tol, max_iter=5000)
    assert st == 0 and it_ref > 3
    pre = fa.PRECOND_JACOBI if jacobi else fa.PRECOND_IDENTITY
    for kernel in _kernels(h["p"].max_row):
        with _kernel(engine, kernel, h["p"].max_row):
            x = np.zeros(h["n"])
            it = engine.cg_solve(values, b, x, pre, rel_tol=tol, max_iter=5000)
            assert engine.last_kernel_name() == kernel
            x2 = np.zeros(h["n"])
            it2 = engine.cg_solve(values, b, x2, pre, rel_tol=tol, max_iter=5000)
        assert abs(it - it_ref) <= max(3, it_ref // 20), (kernel, it, it_ref)
        assert np.linalg.norm(b - a @ x) <= 2 * tol * np.linalg.norm(b)
        assert np.linalg.norm(x - x_ref) <= 1e-7 * np.linalg.norm(x_ref)
        assert it2 == it and np.array_equal(x, x2)          # ordered reductions: bitwise reproducible


# ---- 5. Dirichlet rows and right-hand side, bit-exact
def _node_lists(p):
    N = p.num_nodes
    leaves = list(range(1, N))
    return {"hub": [0], "leaves": leaves, "hub+every second leaf": [0] + leaves[::2], "all": list(range(N)), "none": [],
            "duplicates": [0, 3, 3, 0, N - 1, 3, 1, N - 1]}


def _dirichlet(engine, oracle, torch, h, S, values, nodes):
    ref = values.copy()
    oracle.apply_homogeneous_dirichlet_bc_csr(h["ro"], h["ci"], ref, nodes, S)
    v = torch.from_numpy(values).cuda()
    engine.apply_dirichlet_csr_dev(v, nodes)
    return v.cpu().numpy(), ref


@pytest.mark.gpu
@pytest.mark.parametrize("S", SDIMS)
@pytest.mark.parametrize("name", DIRICHLET)
def test_dirichlet_rows_match_oracle_bitwise(engine, oracle, name, S):
    """every value is kept, zeroed or set to the scale: equal bit for bit to the reference's walk over the scalar CSR, on non-symmetric values"""
    import torch

    h = _bind(engine, name, S)
    rng = _seed("dirichlet", name, S)
    values = rng.standard_normal(len(h["ci"]))
    for label, nodes in _node_lists(h["p"]).items():
        got, ref = _dirichlet(engine, oracle, torch, h, S, values, nodes)
        bad = np.nonzero(got != ref)[0]
        assert np.array_equal(got, ref), (label, len(bad), bad[:6], got[bad[:6]], ref[bad[:6]])
        if nodes:
            assert np.count_nonzero(got != values) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("S", SDIMS)
@pytest.mark.parametrize("name", ["star16", "star33", "star130"])
def test_dirichlet_scale_is_the_first_nonzero_diagonal(engine, oracle, name, S):
    import torch

    h = _bind(engine, name, S)
    rng = _seed("scale", name, S)
    base = rng.standard_normal(len(h["ci"]))
    dpos = cr.diagonal_positions(h["ro"], h["ci"])
    n = h["n"]
    nodes = _node_lists(h["p"])["hub+every second leaf"]
    cases = {}
    for first in (5, n - 1):                          # the leading diagonal entries zero
        v = base.copy()
        v[dpos[:first]] = 0.0
        cases[f"first nonzero diagonal in row {first}"] = (v, abs(base[dpos[first]]))
    v = base.copy()
    v[dpos[0]] = -2.5
    cases["negative first diagonal"] = (v, 2.5)
    v = base.copy()
    v[dpos] = 0.0
    cases["no nonzero diagonal"] = (v, 1.0)
    for label, (v, scale) in cases.items():
        got, ref = _dirichlet(engine, oracle, torch, h, S, v, nodes)
        assert np.array_equal(got, ref), label
        assert got[dpos[0]] == scale and ref[dpos[0]] == scale, (label, got[dpos[0]], scale)


@pytest.mark.gpu
@pytest.mark.parametrize("S", SDIMS)
def test_dirichlet_rhs_on_device(engine, S):
    import torch

    h = _bind(engine, "star130", S)
    N = h["p"].num_nodes
    rng = _seed("rhs", S)
    v = rng.standard_normal(h["n"])
    for count in (1, 255, 256, 257):
        nodes = rng.integers(0, N, size=count)
        if count > N:
            assert len(set(nodes.tolist())) < count           # duplicates
        t = torch.from_numpy(v).cuda()
        engine.apply_dirichlet_rhs_dev(t, nodes)
        assert np.array_equal(t.cpu().numpy(), cr.dirichlet_rhs(v, nodes, S)), count
    for nodes in ([3, 3, 7, 3], []):
        t = torch.from_numpy(v).cuda()
        engine.apply_dirichlet_rhs_dev(t, nodes)
        assert np.array_equal(t.cpu().numpy(), cr.dirichlet_rhs(v, nodes, S))
    t = torch.from_numpy(v).cuda()
    with pytest.raises(fa.FenrisError):
        engine.apply_dirichlet_rhs_dev(t, [1, N, 2])              # one node out of range: nothing is written
    assert np.array_equal(t.cpu().numpy(), v)
