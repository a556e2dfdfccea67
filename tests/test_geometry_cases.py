"""Host only: the entry-wise scale of hp_reference.Reference against a brute-force loop, and every case of geometry_cases.py against what its
name claims -- the aspect ratio or cond J, the sign of det J, the size ratio, how many Hex8 elements the device's classifier will find
affine -- and the reference against itself: evaluated in double it stays within 1 / 64 of the bar that test_extreme_geometry.py holds the
device to, entry by entry, so the long-double values the device is compared with are right far beyond that bar."""
import numpy as np
import pytest

import geometry_cases as gc
import hp_reference as hp

BAR = 1e-12
MU, LAM, RHO = 3.0e2, 5.0e2, 2.5
CASES = gc.all_cases()


def _ids(cases):
    return ["-".join(c) for c in cases]


def _reference(c, model, dt, u=None):
    n = c.mesh.num_nodes() * (1 if model == "LAPLACE" else c.mesh.vertices.shape[1])
    return hp.Reference(c.kind, model, c.mesh.vertices, c.mesh.connectivity, c.w, c.p, np.zeros(n) if u is None else u, MU, LAM, rho=RHO, dt=dt)


# ---- term_scale against a loop over one element, written out index by index
def _brute_force_scale(kind, model, X, w, p, mu, lam):
    n, d = hp.KINDS[kind]
    s = 1 if model == "LAPLACE" else d
    T = np.zeros((n * s, n * s), dtype=np.longdouble)
    X = X.astype(np.longdouble)
    for wq, xi in zip(w, p.reshape(-1, d)):
        _, G = hp.shape(kind, xi)
        J = np.zeros((d, d), dtype=np.longdouble)
        for a in range(n):
            for i in range(d):
                for j in range(d):
                    J[i, j] += X[a, i] * G[a, j]
        Ji = hp.inv(J[None])[0]
        ag = np.zeros((n, d), dtype=np.longdouble)
        for a in range(n):
            for j in range(d):
                for k in range(d):
                    ag[a, j] += abs(G[a, k]) * abs(Ji[k, j])
        scale = np.longdouble(wq) * abs(hp.det(J[None])[0])
        for a in range(n):
            for b in range(n):
                dot = sum(ag[a, k] * ag[b, k] for k in range(d))
                if model == "LAPLACE":
                    T[a, b] += scale * dot
                    continue
                for i in range(d):
                    for j in range(d):
                        T[s * a + i, s * b + j] += scale * (mu * dot * (i == j) + mu * ag[b, i] * ag[a, j] + lam * ag[a, i] * ag[b, j])
    return T


@pytest.mark.parametrize("model", ["LAPLACE", "LINEAR_ELASTIC", "NEO_HOOKEAN"])
@pytest.mark.parametrize("kind", ["HEX8", "TET4"])
def test_term_scale_against_a_brute_force_loop(kind, model):
    c = gc.case(kind, "jittered", "shear")
    conn = np.asarray(c.mesh.connectivity).astype(np.int64)[5:6]
    ref = hp.Reference(kind, model, c.mesh.vertices, conn, c.w, c.p, np.zeros(3 * c.mesh.num_nodes()), MU, LAM)
    T = ref.term_scale()
    assert T.dtype == np.longdouble and T.shape == (1, ref.s * ref.n, ref.s * ref.n)
    want = _brute_force_scale(kind, model, np.asarray(c.mesh.vertices)[conn[0]], c.w, c.p, np.longdouble(MU), np.longdouble(LAM))
    assert np.abs(T[0] - want).max() <= 1e-17 * np.abs(want).max()
    # (an entry made of one term has T = |K|; NeoHookean at u = 0 reaches the same value through F^-1 = I and ln 1: a few long-double ulps)
    assert np.all(T[0] * (1 + np.longdouble(1e-17)) >= np.abs(ref.ke[0]))


@pytest.mark.parametrize("kind,variant,geometry", CASES, ids=_ids(CASES))
def test_the_scale_bounds_every_entry(kind, variant, geometry):
    """T_ij >= |K_ij| entry by entry, element by element and assembled; the diagonal and the rows of apply likewise; |M| = M (linear kinds)"""
    c = gc.case(kind, variant, geometry)
    for model in ("LAPLACE", "LINEAR_ELASTIC"):
        ref = _reference(c, model, np.float64)
        assert np.all(ref.term_scale() >= np.abs(ref.ke))
        ro, ci = ref.pattern()
        T = ref.csr_term_scale(ro, ci)
        assert np.all(T >= np.abs(ref.csr_values(ro, ci)))
        assert np.all(ref.diagonal_term_scale() >= np.abs(ref.diagonal()))
        x = np.random.default_rng(2).uniform(-1.0, 1.0, ref.ndof)
        assert np.all(ref.abs_apply_terms(x) >= ref.abs_apply(x) * (1.0 - 1e-14))
        assert np.all(ref.abs_apply_terms(x, 2.0, -3.0) >= ref.abs_apply(x, 2.0, -3.0) * (1.0 - 1e-14))
        g = gc.element_gamma(c)
        assert np.all(ref.csr_term_scale(ro, ci, gamma=g) >= T) and np.all(g >= 1.0)
        if kind not in ("HEX27", "TET10"):
            assert np.array_equal(ref.csr_term_scale(ro, ci, which="M"), ref.csr_values(ro, ci, which="M"))


# ---- the cases are what they are called
CLAIMS = {"unit": 1.0, "plate_1e2": 1e2, "plate_1e4": 1e4, "needle_1e3": 1e3, "shear": float(np.linalg.cond(gc.SHEAR)), "shifted": 1.0,
          "scaled_down": 1.0, "scaled_up": 1.0, "mirrored": 1.0, "threshold": 1e2}


@pytest.mark.parametrize("kind,variant,geometry", CASES, ids=_ids(CASES))
def test_case_is_what_its_name_says(kind, variant, geometry):
    c = gc.case(kind, variant, geometry)
    pr = gc.properties(c)
    d = c.linear.vertices.shape[1]
    # a simplex of the uniform mesh is not equilateral: its own cond J (and a jitter of 0.1 h) is measured on the unit case, the claim
    # is the factor the map adds
    own = gc.properties(gc.case(kind, variant, "unit")).aspect
    assert own <= (1.6 if kind in ("HEX8", "QUAD4", "HEX27") else 8.0)
    if geometry == "graded":
        # x -> expm1(3 x): the element at x has the size 3 h e^(3 x), from the first to the last one the factor e^(3 (L - h))
        L = float(np.asarray(gc._base(kind)[0].vertices).max())
        want = np.exp(3.0 * (L - c.h))
        assert want / 2.0 <= pr.size_ratio / own <= 2.0 * want and pr.size_ratio >= want / 2.0
    else:
        claim = CLAIMS[geometry] if d == 3 or geometry not in ("plate_1e2", "plate_1e4") else 1.0     # (2D: the plates' thin axis is not there)
        if geometry == "shear" and d == 2:
            claim = float(np.linalg.cond(gc.SHEAR[:2, :2]))
        assert claim / 2.0 <= pr.aspect <= 2.0 * claim * own, (pr.aspect, claim, own)
    assert pr.det_signs == ({-1} if geometry == "mirrored" else {1})
    assert np.linalg.cond(gc.SHEAR) > 30.0 and np.linalg.cond(gc.SHEAR) < 40.0
    X = np.asarray(c.linear.vertices)
    if geometry == "shifted":
        assert np.abs(X).max() >= 2048.0 and np.all(gc.element_gamma(c) >= 2048.0 / (c.h * 2.0))
        if variant == "exact" and kind == "HEX8":   # every coordinate is a multiple of 1 / 8 below 2^12: no rounding at all
            assert np.array_equal(X * 8.0, np.rint(X * 8.0))
    if geometry in ("scaled_down", "scaled_up"):
        unit = np.asarray(gc.case(kind, variant, "unit").linear.vertices)
        assert np.array_equal(X, unit * (2.0 ** -20 if geometry == "scaled_down" else 2.0 ** 20))      # exact: a power of two


HEX8_CASES = [c for c in CASES if c[0] == "HEX8"]


@pytest.mark.parametrize("kind,variant,geometry", HEX8_CASES, ids=_ids(HEX8_CASES))
def test_predicted_affine_classification(kind, variant, geometry):
    c = gc.case(kind, variant, geometry)
    E = c.mesh.num_elements()
    assert E == 378
    n = gc.predicted_affine_elements(c)
    assert n == (E // 2 if geometry == "threshold" else E if variant == "exact" else 0), (n, E)
    if geometry == "threshold":
        # the mixed coefficient of the elements sits a factor 2 inside and outside the tolerance: a classifier that measured against another
        # edge than the shortest (the in-plane ones are 100 times longer) would find all 378 affine
        flags = gc.classify_affine_hex8(c.linear.vertices, c.linear.connectivity)
        assert int(gc.classify_affine_hex8(c.linear.vertices, c.linear.connectivity, 0.3 * gc.AFFINE_TOL).sum()) == 0
        assert int(gc.classify_affine_hex8(c.linear.vertices, c.linear.connectivity, 3.0 * gc.AFFINE_TOL).sum()) == E
        z = np.asarray(c.linear.vertices)[np.asarray(c.linear.connectivity).astype(np.int64)][:, :, 2].mean(axis=1)
        layer = np.floor(z / (1e-2 * c.h)).astype(int)
        assert np.array_equal(flags, layer % 2 == 0)


# ---- the reference alone holds the bar with room
@pytest.mark.parametrize("kind,variant,geometry", CASES, ids=_ids(CASES))
def test_reference_in_double_is_within_a_64th_of_the_bar(kind, variant, geometry):
    c = gc.case(kind, variant, geometry)
    gamma = gc.gamma_of(c)
    bar = BAR / 64.0
    for model in ("LAPLACE", "LINEAR_ELASTIC"):
        s = 1 if model == "LAPLACE" else c.mesh.vertices.shape[1]
        rng = np.random.default_rng(5)
        x = rng.uniform(-1.0, 1.0, s * c.mesh.num_nodes())
        u = gc.smooth_u(np.asarray(c.mesh.vertices), s)
        lo, hi = _reference(c, model, np.float64, u), _reference(c, model, np.longdouble, u)
        ro, ci = hi.pattern()
        T = hi.csr_term_scale(ro, ci, gamma=gamma)
        assert np.all(np.abs(lo.csr_values(ro, ci) - hi.csr_values(ro, ci)) <= bar * T)
        assert np.all(np.abs(lo.diagonal() - hi.diagonal()) <= bar * hi.diagonal_term_scale(gamma=gamma))
        assert np.all(np.abs(lo.apply(x)[0] - hi.apply(x)[0]) <= bar * hi.abs_apply_terms(x, gamma=gamma))
        assert np.all(np.abs(lo.residual() - hi.residual()) <= bar * hi.abs_apply_terms(u, gamma=gamma))    # (r = K u)
        # r = K u indeed: the residual of the linear operators is the apply
        assert np.all(np.abs(hi.residual() - hi.apply(u)[0]) <= 1e-17 * hi.abs_apply_terms(u))
        M = hi.csr_term_scale(ro, ci, which="M", gamma=gamma)
        assert np.all(np.abs(lo.csr_values(ro, ci, "M") - hi.csr_values(ro, ci, "M")) <= bar * M)
        assert np.all(np.abs(lo.apply(x, 1.0, 0.0)[0] - hi.apply(x, 1.0, 0.0)[0]) <= bar * hi.abs_apply_terms(x, 1.0, 0.0, gamma=gamma))
