"""Augmented-Lagrangian contact (fh_set_contact_multipliers, fh_contact_multiplier_update, fenris_amd.AugmentedLagrangian) against the NumPy
statement of tests/augmented_contact_reference.py, which is pinned here on the CPU against central differences of its own energy and force
and, with s = 0, against contact_reference.py bit for bit.  Meshes, problems and bars are those of tests/test_contact.py (and, for the
friction and grid pieces, of tests/test_friction.py and tests/test_sdf_grid.py).

Bounds.  The term is a short sum per node: 1e-13 max|.| (test_contact.SHORT_SUM).  Where an outer loop of Newton solves is compared, the
bound is measured from the reference alone as test_contact._newton_tolerances measures it: d_perm, the reference loop under another element
order, d_newton, the reference loop under a Newton tolerance 100 times smaller, and the bound max(20 (d_perm + d_newton), 1e-13), relative
to max|u|.  A multiplier and a max_change are lengths read off u, so they carry the same bound times max|u| (times 2: a difference of two)."""
import functools
import os

import numpy as np
import pytest

import fenris_amd as fa
from fenris_amd import _ffi

import augmented_contact_reference as ar
import contact_reference as cr
import dynamics_reference as dr
import motion_reference as mr
import sdf_grid_reference as sg
import test_contact as tc
import test_sdf_grid as ts
from test_contact import FH_BAD_ARGUMENT, FH_INVALID_STATE, RHO, SHORT_SUM, engine  # noqa: F401  (engine: the fixture)

NEW = ("fh_set_contact_multipliers", "fh_set_contact_multipliers_dev", "fh_contact_multipliers", "fh_contact_multipliers_dev",
       "fh_contact_multiplier_forces_dev", "fh_contact_multiplier_update")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AL_TOL = 1e-10
_rel, _check, _code = tc._rel, tc._check, tc._code


# ------------------------------------------------------------------------------------------ scenes
def _four_kinds(d):
    """half-space, ball, cavity and a random grid whose box covers part of the mesh (last: sdf_grid_reference sums the grids last)"""
    return tc._three_kinds(d) + [ts._random_grid(d)]


def _random_s(obstacles, X, u, seed=21):
    """multipliers per (obstacle, node): a third zero, a third small, a third large enough to activate a separated node, so that
    phi_eff = phi - s has active pairs that phi alone leaves inactive; every pair 1e-6 clear of phi_eff = 0"""
    rng = np.random.default_rng(seed)
    phi = cr.phi_table(obstacles, X, u)
    s = rng.uniform(0.0, 0.05, phi.shape) * rng.choice([0.0, 1.0, 20.0], phi.shape)
    fin = np.isfinite(phi)
    close = fin & (np.abs(np.where(fin, phi, 0.0) - s) < 1e-6)
    s[close] += 1e-3
    return s


def _assert_s_scene(obstacles, X, u, s):
    phi = cr.phi_table(obstacles, X, u)
    fin = np.isfinite(phi)
    eff = np.where(fin, phi, 1.0) - s
    assert np.abs(eff[fin]).min() >= 1e-6
    for o in range(len(obstacles)):
        row = fin[o]
        assert ((phi[o] > 0) & (eff[o] < 0) & row).sum() >= 1, o          # a separated node the multiplier activates
        assert ((eff[o] > 0) & row).sum() >= 1 and ((eff[o] < 0) & row).sum() >= 3 and (s[o] == 0.0).sum() >= 3, o


# ------------------------------------------------------------------------------------------ 1: declarations
def test_multiplier_entry_points_are_declared():
    hdr = open(os.path.join(ROOT, "include", "fenris_hip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "fenris_hip_sys.rs")).read()
    for name in NEW:
        assert name in _ffi.exported_symbols() and name + "(" in hdr and f"pub fn {name}(" in rs, name
    assert "} fh_multiplier_update;" in hdr and "pub struct fh_multiplier_update {" in rs
    assert [f[0] for f in _ffi.MultiplierUpdateStats._fields_] == ["max_change", "max_penetration", "max_force", "active"]
    for name in ("multipliers", "set_multipliers", "multiplier_forces", "update_multipliers"):
        assert callable(getattr(fa.Contact, name))
    assert callable(fa.AugmentedLagrangian.solve) and issubclass(fa.AugmentedLagrangianError, Exception)
    assert {"max_change", "max_penetration", "active", "max_force"} <= set(fa.MultiplierUpdate.__dataclass_fields__)
    assert {"updates", "multiplier_updates", "newton_results", "converged"} <= set(fa.AugmentedLagrangianResult.__dataclass_fields__)


# ------------------------------------------------------------------------------------------ 2, 3: the reference pinned
@pytest.mark.parametrize("kind", ["HEX8", "QUAD4", "HEX8_3"])
def test_reference_force_is_the_derivative_of_the_energy(kind):
    """g against central differences of E_c with s frozen: the four kinds together, random u of size 0.02, random s (step and bar of
    test_contact's twin)"""
    m = tc._mesh(kind)[0]
    obs = _four_kinds(m.vertices.shape[1])
    u = tc._random_u(m)
    s = _random_s(obs, m.vertices, u)
    _assert_s_scene(obs, m.vertices, u, s)
    g = ar.force(obs, m.vertices, u, s)
    h = 1e-6
    fd = np.zeros_like(g)
    for i in range(len(u)):
        e = np.zeros_like(u)
        e[i] = h
        fd[i] = (ar.energy(obs, m.vertices, u + e, s) - ar.energy(obs, m.vertices, u - e, s)) / (2 * h)
    _check(f"{kind} g vs dE_c", _rel(fd, g), 2e-9)


@pytest.mark.parametrize("kind", ["HEX8", "QUAD4", "HEX8_3"])
def test_reference_exact_tangent_is_the_derivative_of_the_force(kind):
    m = tc._mesh(kind)[0]
    obs = _four_kinds(m.vertices.shape[1])
    u = tc._random_u(m)
    s = _random_s(obs, m.vertices, u)
    _assert_s_scene(obs, m.vertices, u, s)
    # (clear of the grid's cell faces too, where its gradient has a kink)
    assert all(c >= 1e-5 for _, c in sg.cell_clearance(obs, m.vertices, u))
    B = ar.tangent(obs, m.vertices, u, s, exact=True).toarray()
    h = 1e-6
    fd = np.zeros_like(B)
    for i in range(len(u)):
        e = np.zeros_like(u)
        e[i] = h
        fd[:, i] = (ar.force(obs, m.vertices, u + e, s) - ar.force(obs, m.vertices, u - e, s)) / (2 * h)
    _check(f"{kind} B vs dg", _rel(fd, B), 2e-9)


@pytest.mark.parametrize("kind", ["HEX8", "QUAD4"])
def test_reference_applied_tangent_is_positive_semidefinite(kind):
    m = tc._mesh(kind)[0]
    u = tc._random_u(m, seed=3)
    for ob in _four_kinds(m.vertices.shape[1]):
        s = _random_s([ob], m.vertices, u)
        B = ar.blocks([ob], m.vertices, u, s, exact=False)
        assert np.abs(B).max() > 0.0
        assert np.abs(B - B.transpose(0, 2, 1)).max() <= 1e-12 * ob[3]
        assert min(np.linalg.eigvalsh(b).min() for b in B) >= -1e-12 * ob[3] * max(1.0, np.abs(B).max() / ob[3]), ob[0]


@pytest.mark.parametrize("kind", ["HEX8", "QUAD4"])
def test_reference_with_zero_multipliers_is_contact_reference(kind):
    """s = 0 (and s None): every quantity array_equal to contact_reference's (the three kinds) and sdf_grid_reference's (with the grid)"""
    m = tc._mesh(kind)[0]
    X, u = m.vertices, tc._random_u(m)
    w = np.random.default_rng(8).uniform(0.5, 2.0, len(X))
    three, four = tc._three_kinds(X.shape[1]), _four_kinds(X.shape[1])
    for s in (None, np.zeros((3, len(X)))):
        assert ar.energy(three, X, u, s, w) == cr.energy(three, X, u, w)
        assert np.array_equal(ar.force(three, X, u, s, w), cr.force(three, X, u, w))
        for exact in (False, True):
            assert np.array_equal(ar.blocks(three, X, u, s, w, exact), cr.blocks(three, X, u, w, exact))
    assert ar.energy(four, X, u, None, w) == sg.energy(four, X, u, w)
    assert np.array_equal(ar.force(four, X, u, None, w), sg.force(four, X, u, w))
    for exact in (False, True):
        assert np.array_equal(ar.blocks(four, X, u, None, w, exact), sg.blocks(four, X, u, w, exact))
    # friction: the lag state of test_sdf_grid's scene, zero multipliers against friction_reference
    import friction_reference as fr

    rng = np.random.default_rng(31)
    ubar = rng.uniform(-0.02, 0.02, X.size)
    d = rng.uniform(-0.02, 0.02, X.size)
    mu = [0.5, 0.3, 0.7, 0.2]
    assert np.array_equal(ar.friction_force(three, mu[:3], X, ubar, d, ts.EPS, None, w), fr.force(three, mu[:3], X, ubar, d, ts.EPS, w))
    assert ar.friction_potential(three, mu[:3], X, ubar, d, ts.EPS, None, w) == fr.potential(three, mu[:3], X, ubar, d, ts.EPS, w)
    # (a grid's lam is k w (-phi) |m| here and k w (-(phi |m|)) there: equal to rounding, not to the bit)
    assert _rel(ar.friction_force(four, mu, X, ubar, d, ts.EPS, None, w), fr.force(four, mu, X, ubar, d, ts.EPS, w)) <= 1e-15
    assert ar.multiplier_forces(four, X, u, None, w).any() == False  # noqa: E712


def test_reference_update():
    """s stays >= 0, a node outside a grid's box gets 0, a separated node's multiplier is released in one update, an active one grows by its
    penetration; skip nodes keep 0 and stay out of the statistics"""
    m = tc._mesh("HEX8")[0]
    X, u = m.vertices, tc._random_u(m)
    obs = _four_kinds(3)
    s = _random_s(obs, X, u)
    phi = cr.phi_table(obs, X, u)
    new, st = ar.update(obs, X, u, s)
    assert (new >= 0.0).all() and np.isfinite(new).all()
    outside = np.isinf(phi[3])
    assert outside.sum() >= 3 and (s[3][outside] > 0).any() and not new[3][outside].any()
    released = (phi > 0) & (s > 0) & (s < phi)
    assert released.sum() >= 3 and not new[released].any()
    grown = np.isfinite(phi) & (phi < 0)
    assert np.array_equal(new[grown], s[grown] - phi[grown]) and (new[grown] > s[grown]).all()
    assert st["max_change"] == np.abs(new - s).max() and st["max_penetration"] == -phi[np.isfinite(phi)].min() and st["active"] == (new > 0).sum()
    again, st2 = ar.update(obs, X, u, new)          # the separated ones stay released
    assert not again[released].any()
    deepest = int(np.argmin(np.where(np.isfinite(phi), phi, 0.0).min(axis=0)))
    skipped, st3 = ar.update(obs, X, u, s, skip=[deepest])
    assert not skipped[:, deepest].any() and st3["max_penetration"] < st["max_penetration"]
    # from nothing: one update of a pure penalty state gives s = the penetration
    first, _ = ar.update(obs, X, u)
    assert np.array_equal(first, np.maximum(0.0, -np.where(np.isfinite(phi), phi, 1.0)))


# ------------------------------------------------------------------------------------------ the seated block: scene, reference loop
SEAT_K, SEAT_F = 1.0e4, 2.0
SEAT_FLOOR = [("half_space", (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), SEAT_K)]
NEWTON_TOLERANCE = tc.NEWTON_TOLERANCE


def _seat(kind, rollers="xy"):
    """a unit cube on the floor z >= 0 under a dead load SEAT_F spread over the nodes of its top face; no support in z but the floor;
    rollers: u_x held on the face x = 0 ("x") and u_y on the face y = 0 ("y") take the rigid modes"""
    m = tc._mesh(kind)[0]
    top, bottom = tc._face(m, 2, 1.0), tc._face(m, 2, 0.0)
    f = np.zeros(m.vertices.size)
    f[3 * top + 2] = -SEAT_F / len(top)
    dofs = [(tc._face(m, a, 0.0), [a]) for a in range(2) if "xy"[a] in rollers]
    return m, top, bottom, f, dofs


def _seat_guess(m, bottom):
    """the uniform penetration at which the penalty alone carries the load: at u = 0 the bottom nodes are ON the floor, inactive, and nothing
    holds the block in z"""
    u0 = np.zeros(m.vertices.size)
    u0[2::3] = -SEAT_F / (SEAT_K * len(bottom))
    return u0


def _hold(prob, dofs):
    for nodes, comps in dofs:
        for c in comps:
            prob.free[3 * np.asarray(nodes, dtype=np.int64) + c] = False
    return prob


@functools.lru_cache(maxsize=None)
def _seat_reference(kind, op, perm=None, tol=NEWTON_TOLERANCE, load=1.0):
    from oracle import oracle as o

    o.lib()
    m, top, bottom, f, dofs = _seat(kind)
    aug = ar.AugmentedProblem(_hold(tc._problem(o, kind, op, SEAT_FLOOR, perm=perm), dofs))
    u, hist, ok = ar.augmented_lagrangian(aug, load * f, _seat_guess(m, bottom), tol, 30, AL_TOL)
    return u, hist, ok, aug


def _assert_margins(hist):
    """the scene decides nothing on a rounding: no max_change within a factor 1.5 of the tolerance, no pair within 1e-8 of switching"""
    for h in hist:
        assert not AL_TOL / 1.5 < h["max_change"] < 1.5 * AL_TOL, h["max_change"]
        assert h["margin"] >= 1e-8, h["margin"]


def _loop_bound(ref_of):
    """(reference, bound) of an outer loop: ref_of(perm, tol) -> (u, history, converged, ...)"""
    ref = ref_of(None, NEWTON_TOLERANCE)
    d_perm = _rel(ref_of(7, NEWTON_TOLERANCE)[0], ref[0])
    d_newton = _rel(ref_of(None, NEWTON_TOLERANCE / 100.0)[0], ref[0])
    bound = max(20.0 * (d_perm + d_newton), 1e-13)
    print(f"d_perm {d_perm:.2e} d_newton {d_newton:.2e} bound {bound:.2e}")
    return ref, bound


@pytest.mark.parametrize("kind,op", [("HEX8_3", "elastic"), ("HEX8_3", "neo_hookean"), ("TET4", "elastic"), ("TET4", "neo_hookean")])
def test_reference_seated_block_converges(kind, op):
    """the condition on the scene: with k = SEAT_K the reference loop alone reaches max_change <= 1e-10 within 30 updates; update 0 sees
    the penalty's penetration (k times its sum over the bottom nodes carries the load), the last one none"""
    u, hist, ok, aug = _seat_reference(kind, op)
    m, top, bottom, f, dofs = _seat(kind)
    print(kind, op, [f"{h['max_change']:.2e}" for h in hist])
    assert ok and len(hist) <= 30 and hist[-1]["max_change"] <= AL_TOL
    _assert_margins(hist)
    pen0 = np.maximum(0.0, -cr.phi_table(SEAT_FLOOR, m.vertices, hist[0]["u"])[0])
    assert abs(SEAT_K * pen0.sum() - SEAT_F) <= 1e-9 * SEAT_F and hist[0]["max_penetration"] >= SEAT_F / (SEAT_K * len(bottom))
    assert hist[-1]["max_penetration"] <= AL_TOL
    assert abs(ar.resultants(SEAT_FLOOR, m.vertices, u, aug.s)[0][2] + SEAT_F) <= 1e-9 * SEAT_F


# ------------------------------------------------------------------------------------------ GPU helpers
def _solver(engine, kind, op, obstacles, f, dofs=(), nodes=None):
    asm = tc._assembler(engine, kind, op)
    newton = fa.MatrixFreeNewton(asm)
    if nodes is not None:
        newton.with_dirichlet_nodes(nodes)
    for nd, comps in dofs:
        newton.with_dirichlet_dofs(nd, comps)
    return newton.with_load(f).with_obstacles(obstacles)


NEWTON_KW = dict(line_search=fa.BacktrackingLineSearch(), preconditioner=_ffi.PRECOND_JACOBI, linear_rel_tol=1e-13)


def _set_u(engine, kind, op, u):
    return tc._assembler(engine, kind, op, u)


# ------------------------------------------------------------------------------------------ 4: term parity with multipliers standing
def _parity_scene(kind):
    X = np.asarray(tc._mesh(kind)[0].vertices)
    N, d = X.shape
    obs = _four_kinds(d)
    paths = [([0.0, 2.0], [[0.0] * d, [0.03125, -0.015625, 0.0078125][:d]]), None, None, None]     # the half-space moves
    t = 1.25
    rng = np.random.default_rng(31)
    w = rng.uniform(0.5, 2.0, N)
    ubar = rng.uniform(-0.02, 0.02, N * d)
    u = ubar + (rng.uniform(-0.02, 0.02, (N, d)) * rng.choice([0.1, 1.0], (N, 1))).reshape(-1)
    cur = mr.placed(obs, paths, t)
    s = _random_s(cur, X, u)
    lag_phi = cr.phi_table(cur, X, ubar)
    fin = np.isfinite(lag_phi)
    close = fin & (np.abs(np.where(fin, lag_phi, 0.0) - s) < 1e-6)
    s[close] += 1e-3
    return obs, paths, t, w, ubar, u, s, cur


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["HEX8", "QUAD4", "TET4", "TET10"])
def test_term_parity_with_multipliers(engine, kind):
    """energy, gap (geometric), force, CSR blocks, the tangent's map and diagonal, resultants, multiplier forces, the friction potential, force
    and resultants, and one update with its four statistics, against the reference: the four kinds together with node weights, the
    half-space on a path at the clock 1.25, random multipliers (zeros, small ones, ones that activate separated nodes)"""
    import torch

    obs, paths, t, w, ubar, u, s, cur = _parity_scene(kind)
    mu = [0.5, 0.3, 0.7, 0.2]
    m = tc._mesh(kind)[0]
    X = np.asarray(m.vertices)
    n, d = X.size, X.shape[1]
    _assert_s_scene(cur, X, u, s)
    asm = tc._assembler(engine, kind, "neo_hookean", u)
    con = fa.Contact(engine)

    def arm(mu_=None, **kw):
        engine.set_obstacles(ts._fa_obstacles(obs, mu_, paths, w, **kw))
        engine.set_obstacle_time(t, t)
        con.set_multipliers(s)

    arm()
    assert np.array_equal(con.multipliers(), s)
    e_ref, g_ref = ar.energy(cur, X, u, s, w), ar.force(cur, X, u, s, w)
    B_ref = ar.tangent(cur, X, u, s, w).toarray()
    assert np.abs(g_ref - sg.force(cur, X, u, w)).max() > 1e-3 * np.abs(g_ref).max()       # the multipliers show
    _check(f"{kind} energy", abs(con.energy() - e_ref) / abs(e_ref), SHORT_SUM)
    gap, gap_ref = con.gap(), sg.gap(cur, X, u)
    assert np.array_equal(np.isinf(gap), np.isinf(gap_ref))
    _check(f"{kind} gap stays geometric", _rel(gap[np.isfinite(gap_ref)], gap_ref[np.isfinite(gap_ref)]), SHORT_SUM)
    _check(f"{kind} force", _rel(con.force(), g_ref), SHORT_SUM)
    _check(f"{kind} csr blocks", np.abs(tc._csr_of_contact(engine, asm) - B_ref).max() / np.abs(B_ref).max(), SHORT_SUM)
    R_ref = ar.resultants(cur, X, u, s, w)
    _check(f"{kind} resultants", _rel(con.resultants()[0], R_ref), SHORT_SUM)
    _check(f"{kind} multiplier forces", _rel(con.multiplier_forces(), ar.multiplier_forces(cur, X, u, s, w)), SHORT_SUM)
    assert engine.last_kernel_name() == "k_contact_multiplier_forces"
    # the tangent's map and diagonal with the obstacles and multipliers minus the same without
    x = np.random.default_rng(6).uniform(-1.0, 1.0, n)
    tan = fa.MatrixFreeTangent(asm).with_obstacles(ts._fa_obstacles(obs, None, paths, w))
    engine.set_obstacle_time(t, t)
    con.set_multipliers(s)
    y1 = tan.apply(np.zeros(n), x).copy()
    route = engine.last_kernel_name()
    d1 = tan.diagonal()
    tan.with_obstacles(None)
    y0, d0 = tan.apply(np.zeros(n), x).copy(), tan.diagonal()
    _check(f"{kind} apply difference", np.abs((y1 - y0) - B_ref @ x).max() / max(np.abs(B_ref @ x).max(), np.abs(y0).max()), SHORT_SUM)
    _check(f"{kind} diagonal difference", np.abs((d1 - d0) - B_ref.diagonal()).max() / np.abs(d1).max(), SHORT_SUM)
    assert route.endswith("+ k_contact_apply" if kind == "TET10" else "k_operator_from_partials"), route
    # friction at the lag state, with the multipliers that stand
    arm(mu, slip_length=ts.EPS)
    engine._check(engine._lib.fh_set_friction_reference(engine._h, _ffi.fp(np.ascontiguousarray(ubar))))
    assert np.array_equal(con.multipliers(), s)                   # (fh_set_friction* leave them)
    fargs = (cur, mu, X, ubar, u - ubar, ts.EPS, s, w)
    q_ref = ar.friction_force(*fargs)
    assert np.abs(q_ref - ar.friction_force(*fargs[:6], None, w)).max() > 1e-3 * np.abs(q_ref).max()
    D_ref = ar.friction_potential(*fargs)
    _check(f"{kind} friction potential", abs(con.friction_potential() - D_ref) / abs(D_ref), SHORT_SUM)
    _check(f"{kind} friction force", _rel(con.friction_force(), q_ref), SHORT_SUM)
    H_ref = np.zeros_like(B_ref)
    for i, h in enumerate(ar.friction_blocks(*fargs)):
        H_ref[d * i:d * i + d, d * i:d * i + d] = h
    _check(f"{kind} csr blocks with friction", np.abs(tc._csr_of_contact(engine, asm) - (B_ref + H_ref)).max() / np.abs(B_ref + H_ref).max(), SHORT_SUM)
    _check(f"{kind} friction resultants", _rel(con.resultants()[1], ar.friction_resultants(*fargs)), SHORT_SUM)
    # one update, twice from the same state: the same bits; the skip nodes
    arm()
    up = con.update_multipliers()
    assert engine.last_kernel_name() == "k_contact_multiplier_update"
    new = con.multipliers()
    new_ref, st = ar.update(cur, X, u, s, w)
    assert np.array_equal(new > 0, new_ref > 0) and (new >= 0).all()
    _check(f"{kind} update", _rel(new, new_ref), SHORT_SUM)
    for name, got in (("max_change", up.max_change), ("max_penetration", up.max_penetration), ("max_force", up.max_force)):
        _check(f"{kind} {name}", abs(got - st[name]) / st[name], SHORT_SUM)
    assert up.active == st["active"]
    con.set_multipliers(s)
    up2 = con.update_multipliers()
    assert np.array_equal(con.multipliers(), new) and up2 == up
    skip = np.array([0, len(X) - 1])
    con.set_multipliers(s)
    up3 = con.update_multipliers(skip)
    new3 = con.multipliers()
    ref3, st3 = ar.update(cur, X, u, s, w, skip)
    assert not new3[:, skip].any() and up3.active == st3["active"]
    _check(f"{kind} update with skip nodes", _rel(new3, ref3), SHORT_SUM)
    _check(f"{kind} max_change with skip nodes", abs(up3.max_change - st3["max_change"]) / st3["max_change"], SHORT_SUM)
    # a device tensor goes in as it is
    con.set_multipliers(torch.tensor(s, device="cuda:0"))
    assert np.array_equal(con.multipliers(), s)


# ------------------------------------------------------------------------------------------ 5: the shifted map on every route
@pytest.mark.gpu
@pytest.mark.parametrize("dirichlet", [False, True])
@pytest.mark.parametrize("kind,op,table,kernel", tc.ROUTES)
def test_shifted_map_on_every_route_with_multipliers(engine, oracle, kind, op, table, kernel, dirichlet):
    """(M + beta (K + B)) x and its diagonal with multipliers standing, on the routes and at the bar of test_contact's twin"""
    m, w, p = tc._mesh(kind)
    d = m.vertices.shape[1]
    X = np.asarray(m.vertices)
    obs = tc._three_kinds(d)
    u = tc._random_u(m)
    s = _random_s(obs, X, u)
    _assert_s_scene(obs, X, u, s)
    qt, groups = (None, [(np.asarray(m.connectivity), w, p)]) if table == "uniform" else tc._rule_set(kind)
    alpha, beta = 1.0, 0.37
    bc = tc._face(m, 0, 0.0) if dirichlet else np.zeros(0, dtype=np.int64)
    x = np.random.default_rng(9).uniform(-1.0, 1.0, X.size)

    def reference(P):
        def prob_of(Xn, gr, sn):
            return ar.AugmentedProblem(cr.ContactProblem(oracle, tc._okind(kind), tc._oop(oracle, op), Xn, gr, params=tc.LAME.as_pair(), rho=RHO,
                                                         obstacles=obs), sn)

        def dofs(nodes):
            return (d * np.asarray(nodes, dtype=np.int64)[:, None] + np.arange(d)).reshape(-1)

        if P is None:
            prob, un, xn, bcn, inv = prob_of(X, groups, s), u, x, np.asarray(bc, dtype=np.int64), None
        else:
            inv = np.empty_like(P)
            inv[P] = np.arange(len(P))
            gr = [(inv[np.asarray(c, dtype=np.int64)].astype(np.uint64), wq, pq) for c, wq, pq in groups]
            prob, un, xn, bcn = prob_of(X[P], gr, s[:, P]), u[dofs(P)], x[dofs(P)], inv[np.asarray(bc, dtype=np.int64)]
        A = (alpha * prob.mass() + beta * prob.tangent(un)).tocsr()
        diag = A.diagonal()
        fixed = np.zeros(prob.n, dtype=bool)
        if len(bcn):
            fixed[dofs(bcn)] = True
        y = np.asarray(A @ np.where(fixed, 0.0, xn)).reshape(-1)
        first = 0 if inv is None else inv[0] * d
        scale = abs(diag[first])
        assert scale != 0.0
        y, diag = np.where(fixed, scale * xn, y), np.where(fixed, scale, diag)
        if inv is not None:
            y, diag = y[dofs(inv)], diag[dofs(inv)]
        return y, diag

    y_ref, d_ref = reference(None)
    P = np.random.default_rng(10).permutation(len(X))
    P[np.where(P == 0)[0][0]], P[0] = P[0], 0
    y_perm, d_perm_ = reference(P)
    d_perm = max(_rel(y_perm, y_ref), _rel(d_perm_, d_ref))
    tol = max(20.0 * d_perm, 1e-13)
    asm = tc._assembler(engine, kind, op, u, qt)
    t = fa.MatrixFreeShiftedTangent(asm, RHO, alpha, beta).with_dirichlet_nodes(bc if dirichlet else None).with_obstacles(tc._fa_obstacles(obs))
    y_plain = t.apply(np.zeros_like(x), x).copy()
    fa.Contact(engine).set_multipliers(s)
    y = t.apply(np.zeros_like(x), x)
    name = engine.last_kernel_name()
    print(f"{kind} {op} {table} dirichlet={dirichlet}: {name}; d_perm {d_perm:.2e}")
    if kernel is not None:
        assert name == kernel, name
    _check("apply", _rel(y, y_ref), tol)
    _check("diagonal", _rel(t.diagonal(), d_ref), tol)
    assert _rel(y_plain, y_ref) > 1e-3                     # without the multipliers the map differs


# ------------------------------------------------------------------------------------------ 6: zero multipliers, the bits of none
@pytest.mark.gpu
@pytest.mark.parametrize("kind,op", [("HEX8_3", "neo_hookean"), ("TET4", "elastic"), ("TET10", "neo_hookean")])
def test_zero_multipliers_change_no_bit(kind, op):
    """all-zero multipliers, and multipliers set then cleared, give the bits of none: the tangent's map and diagonal, the contact energy, a
    Newton solve, 8 central-difference steps (Tet10: 2 backward-Euler steps), array_equal; and the kernel names do not change"""
    m = tc._mesh(kind)[0]
    X = np.asarray(m.vertices)
    n = X.size
    side = tc._face(m, 2, 1.0)            # the top face held; the floor z >= 0.02 presses the bottom face in, the cavity the eight corners
    x = np.random.default_rng(12).uniform(-1.0, 1.0, n)
    f = np.zeros(n)
    f[0::3] = 0.05
    obs = [("half_space", (0.0, 0.0, 0.02), (0.0, 0.0, 1.0), 2.0e3), ("cavity", (0.5, 0.5, 0.5), 0.85, 5.0e2)]
    u_r = tc._random_u(m)
    rng = np.random.default_rng(13)

    def run(mode):
        eng = fa.Engine(0)
        try:
            asm = tc._assembler(eng, kind, op, u_r)
            con = fa.Contact(eng)

            def arm():
                if mode == "zero":
                    con.set_multipliers(np.zeros((len(obs), len(X))))
                elif mode == "set_then_clear":
                    con.set_multipliers(rng.uniform(0.0, 0.1, (len(obs), len(X))))
                    con.set_multipliers(None)

            t = fa.MatrixFreeTangent(asm).with_dirichlet_nodes(side).with_obstacles(tc._fa_obstacles(obs))
            arm()
            y = t.apply(np.zeros(n), x).copy()
            names = [eng.last_kernel_name()]
            dg = t.diagonal()
            names.append(eng.last_kernel_name())
            e = np.array([con.energy()])
            g = con.force()
            u = np.zeros(n)
            solver = fa.MatrixFreeNewton(asm).with_dirichlet_nodes(side).with_load(f).with_obstacles(tc._fa_obstacles(obs))
            arm()
            res = solver.solve(u, fa.NewtonSettings(40, 1e-9), linear_rel_tol=1e-10)
            names.append(eng.last_kernel_name())
            if kind == "TET10":
                ti = fa.BackwardEuler(asm, RHO, 1e-2).with_newton(fa.NewtonSettings(30, 1e-9), linear_rel_tol=1e-10)
            else:
                ti = fa.CentralDifference(asm, RHO, 1e-3)
            ti.with_dirichlet_nodes(side).with_load(f).with_obstacles(tc._fa_obstacles(obs))
            arm()
            ti.set_state(np.zeros(n), 0.01 * x)
            rec = ti.step(2 if kind == "TET10" else 8, 4)
            names.append(eng.last_kernel_name())
            uu, vv, aa, _, _ = ti.state()
            ti.close()
            return (y, dg, e, g, u, np.array([res.iterations, res.linear_iterations, res.residual_norm]), uu, vv, aa, rec.kinetic, rec.stored), names
        finally:
            eng.close()

    never, names = run("never")
    cleared, names_cleared = run("set_then_clear")
    assert names_cleared == names, (names, names_cleared)
    zero, names_zero = run("zero")
    assert names_zero == names, (names, names_zero)          # (the instantiation is a template argument: the name stays)
    for mode, got in (("set_then_clear", cleared), ("zero", zero)):
        for i, (p, q) in enumerate(zip(never, got)):
            assert np.array_equal(p, q), (mode, i)


# ------------------------------------------------------------------------------------------ 7: the seated block
@pytest.mark.gpu
@pytest.mark.parametrize("kind,op", [("HEX8_3", "elastic"), ("HEX8_3", "neo_hookean"), ("TET4", "elastic"), ("TET4", "neo_hookean")])
def test_seated_block(engine, kind, op):
    """the device's outer loop against the reference's: max_change per update, the final u, the final penetration, the resultant"""
    (u_ref, hist, ok, aug), bound = _loop_bound(lambda perm, tol: _seat_reference(kind, op, perm, tol))
    assert ok
    m, top, bottom, f, dofs = _seat(kind)
    X = np.asarray(m.vertices)
    newton = _solver(engine, kind, op, tc._fa_obstacles(SEAT_FLOOR), f, dofs)
    u = _seat_guess(m, bottom)
    res = fa.AugmentedLagrangian(newton, 30, AL_TOL).solve(u, fa.NewtonSettings(40, NEWTON_TOLERANCE), **NEWTON_KW)
    scale = np.abs(u_ref).max()
    print(f"seated {kind} {op}: reference {len(hist)} updates, device {res.updates}")
    for k, up in enumerate(res.multiplier_updates):
        print(f"  update {k}: max_change {up.max_change:.3e} (reference {hist[k]['max_change']:.3e}) penetration {up.max_penetration:.3e} active {up.active}")
    assert res.converged and res.updates == len(hist) and len(res.newton_results) == res.updates
    for k, up in enumerate(res.multiplier_updates):
        assert abs(up.max_change - hist[k]["max_change"]) <= 2.0 * bound * scale, k
        assert up.active == hist[k]["active"], k
    _check("u", _rel(u, u_ref), bound)
    first, last = res.multiplier_updates[0], res.multiplier_updates[-1]
    assert first.max_penetration >= SEAT_F / (SEAT_K * len(bottom)) and last.max_penetration <= AL_TOL
    con = fa.Contact(engine)
    _check("multipliers", np.abs(con.multipliers() - aug.s).max() / scale, 2.0 * bound)
    R = con.resultants()[0]
    _check("sum R - load", np.abs(R[0] - f.reshape(-1, 3).sum(axis=0)).max(), 10.0 * np.sqrt(X.size) * NEWTON_TOLERANCE)
    lam = con.multiplier_forces()
    assert (lam >= 0.0).all() and abs(lam.sum() - SEAT_F) <= 1e-6 * SEAT_F          # the multipliers alone carry the load


# ------------------------------------------------------------------------------------------ 8: the ball indenter
# pressed 0.0975 deep at k = 600 (chosen on the CPU with the reference alone): the four diagonal neighbours of the centre node are inside the
# ball while the penalty alone lets it sink in, and leave it at the third update as the multipliers push the surface down: 9, 9, 5, 5, ...
BALL = [("ball", (0.5, 0.5, 1.0 + 0.4 - 0.0975), 0.4, 6.0e2)]


@functools.lru_cache(maxsize=None)
def _ball_reference(perm=None, tol=1e-9):
    from oracle import oracle as o

    o.lib()
    kind = "HEX8_6"
    m = tc._mesh(kind)[0]
    bottom = tc._face(m, 2, 0.0)
    aug = ar.AugmentedProblem(tc._problem(o, kind, "neo_hookean", BALL, bottom, perm=perm))
    u, hist, ok = ar.augmented_lagrangian(aug, np.zeros(m.vertices.size), np.zeros(m.vertices.size), tol, 30, AL_TOL, skip=bottom)
    return u, hist, ok, aug


def test_reference_ball_indenter_changes_its_active_set():
    u, hist, ok, aug = _ball_reference()
    sets = [h["active"] for h in hist]
    print("active per update", sets, [f"{h['max_change']:.2e}" for h in hist])
    assert ok and len(set(sets)) >= 2
    _assert_margins(hist)


@pytest.mark.gpu
def test_ball_indenter(engine):
    """a ball pressed 0.0975 into the top face of HEX8_6, Neo-Hookean, the bottom held: the active set changes between updates and is the
    reference's at every update; the final u within the derived bound (Newton tolerance 1e-9 as in test_contact's indenter)"""
    kind = "HEX8_6"
    ref = _ball_reference()
    d_perm = _rel(_ball_reference(7)[0], ref[0])
    d_newton = _rel(_ball_reference(None, 1e-11)[0], ref[0])
    bound = max(20.0 * (d_perm + d_newton), 1e-13)
    print(f"indenter: d_perm {d_perm:.2e} d_newton {d_newton:.2e} bound {bound:.2e}")
    u_ref, hist, ok, aug = ref
    m = tc._mesh(kind)[0]
    bottom = tc._face(m, 2, 0.0)
    n = m.vertices.size
    newton = _solver(engine, kind, "neo_hookean", tc._fa_obstacles(BALL), np.zeros(n), nodes=bottom)
    con = fa.Contact(engine)
    u = np.zeros(n)
    for k, h in enumerate(hist):
        newton.solve(u, fa.NewtonSettings(40, 1e-9), **NEWTON_KW)
        up = con.update_multipliers(bottom)
        s = con.multipliers()
        assert (con.multiplier_forces() >= 0.0).all()
        assert np.array_equal(s > 0.0, h["active_set"]), k
        assert up.active == h["active"]
    assert up.max_change <= AL_TOL and len({h["active"] for h in hist}) >= 2
    _check("u", _rel(u, u_ref), bound)


# ------------------------------------------------------------------------------------------ 9: load, then unload
@pytest.mark.gpu
def test_load_then_unload(engine):
    """the seated block loaded, then the load removed and the loop rerun from the loaded state: every multiplier returns to exactly 0 and u to
    the stress-free state (a rigid lift off the floor at most: no strain, the bottom on or above the floor); lam >= 0 at every update"""
    kind, op = "HEX8_3", "neo_hookean"
    m, top, bottom, f, dofs = _seat(kind)
    X = np.asarray(m.vertices)
    newton = _solver(engine, kind, op, tc._fa_obstacles(SEAT_FLOOR), f, dofs)
    con = fa.Contact(engine)
    u = _seat_guess(m, bottom)
    settings = fa.NewtonSettings(40, NEWTON_TOLERANCE)
    for phase, load in (("load", f), ("unload", np.zeros_like(f))):
        newton.with_load(load)
        for k in range(30):
            newton.solve(u, settings, **NEWTON_KW)
            up = con.update_multipliers()
            assert (con.multiplier_forces() >= 0.0).all() and (con.multipliers() >= 0.0).all(), (phase, k)
            if up.max_change <= AL_TOL:
                break
        assert up.max_change <= AL_TOL, (phase, up)
        print(f"{phase}: {k + 1} updates, active {up.active}, largest force {up.max_force:.3e}")
        if phase == "load":
            assert up.active == len(bottom) and abs(con.multiplier_forces().sum() - SEAT_F) <= 1e-6 * SEAT_F
    assert up.active == 0 and not con.multipliers().any() and up.max_force == 0.0
    uz = u.reshape(-1, 3)
    # stress-free: the residual without the load vanishes and the block is undeformed (a rigid translation in z at most)
    assert np.abs(uz[:, :2]).max() <= 1e-9 and np.ptp(uz[:, 2]) <= 1e-9 and uz[:, 2].min() >= -AL_TOL
    assert con.energy() == 0.0


# ------------------------------------------------------------------------------------------ 10: friction on the true normal force
FRICTION_MU, FRICTION_EPS, WALL_GAP = 0.5, 1.0e-3, 5.0e-3
FRICTION_OBS = SEAT_FLOOR + [("half_space", (1.0 + WALL_GAP, 0.0, 0.0), (-1.0, 0.0, 0.0), SEAT_K)]     # the floor, and a wall beyond x = 1


def _side_load(m, fraction):
    """fraction * mu * SEAT_F in +x over the nodes of the bottom face (at the height of the friction force: no couple tips the block)"""
    bottom = tc._face(m, 2, 0.0)
    f = np.zeros(m.vertices.size)
    f[3 * bottom] = fraction * FRICTION_MU * SEAT_F / len(bottom)
    return f


def _friction_guesses(m, u1, fraction):
    """the lag state of the seating solve: the uniform penetration that carries the load (so that the floor holds the block sideways from
    the first iteration on); the guess of the sheared solve: above the limit the block already at the wall, which carries the excess"""
    bottom, wall = tc._face(m, 2, 0.0), tc._face(m, 0, 1.0)
    u0 = _seat_guess(m, bottom)
    if u1 is None:
        return u0
    guess = np.array(u1)
    if fraction > 1.0:
        guess[0::3] += WALL_GAP + (fraction - 1.0) * FRICTION_MU * SEAT_F / (SEAT_K * len(wall))
    return guess


@functools.lru_cache(maxsize=None)
def _friction_reference(fraction):
    """seat the block (multipliers converged, no side load), move the lag state there, add the side load and run the loop again"""
    from oracle import oracle as o

    o.lib()
    kind, op = "HEX8_3", "elastic"
    m, top, bottom, f, dofs = _seat(kind, rollers="y")
    u0 = _friction_guesses(m, None, fraction)
    aug = ar.AugmentedProblem(_hold(tc._problem(o, kind, op, FRICTION_OBS), dofs), mu=[FRICTION_MU, 0.0], eps=FRICTION_EPS, ubar=u0)
    u1, hist1, ok1 = ar.augmented_lagrangian(aug, f, u0, NEWTON_TOLERANCE, 30, AL_TOL)
    aug.ubar = u1.copy()
    u2, hist2, ok2 = ar.augmented_lagrangian(aug, f + _side_load(m, fraction), _friction_guesses(m, u1, fraction), NEWTON_TOLERANCE, 30, AL_TOL)
    return u1, u2, hist1, hist2, ok1 and ok2, aug


@pytest.mark.parametrize("fraction", [0.5, 1.5])
def test_reference_friction_on_the_seated_block(fraction):
    u1, u2, hist1, hist2, ok, aug = _friction_reference(fraction)
    m, top, bottom, f, dofs = _seat("HEX8_3", rollers="y")
    X = m.vertices
    assert ok
    R = ar.resultants(FRICTION_OBS, X, u2, aug.s)
    Q = ar.friction_resultants(FRICTION_OBS, [FRICTION_MU, 0.0], X, aug.ubar, u2 - aug.ubar, FRICTION_EPS, aug.s)
    slip = (u2 - u1).reshape(-1, 3)[bottom, 0]
    print(f"fraction {fraction}: slip {slip.min():.3e} .. {slip.max():.3e}; |Q| {np.linalg.norm(Q[0]):.4f} mu |R| {FRICTION_MU * np.linalg.norm(R[0]):.4f}")
    bar = 10.0 * np.sqrt(X.size) * NEWTON_TOLERANCE + SEAT_K * len(bottom) * AL_TOL      # (see the device's test)
    assert abs(R[0][2] + SEAT_F) <= bar                                            # the true normal force
    if fraction < 1.0:
        assert np.abs(slip).max() < FRICTION_EPS and abs(Q[0][0] - fraction * FRICTION_MU * SEAT_F) <= FRICTION_MU * bar and not R[1].any()
    else:
        assert slip.min() > FRICTION_EPS and R[1][0] > 0.0
        assert abs(np.linalg.norm(Q[0]) - FRICTION_MU * np.linalg.norm(R[0])) <= 0.05 * FRICTION_MU * np.linalg.norm(R[0])


@pytest.mark.gpu
@pytest.mark.parametrize("fraction", [0.5, 1.5])
def test_friction_on_the_seated_block(engine, fraction):
    """mu = 0.5 on the floor: a side load of half the Coulomb limit and the block sticks (every slip < eps, Q balances the load); 1.5 times the
    limit and it slides until the frictionless wall stops it, with |Q| = mu |R| within the 5 % of test_friction's slide, R the true normal
    force: the load, where the penalty alone reports k times the penetration"""
    kind, op = "HEX8_3", "elastic"
    u1_ref, u2_ref, hist1, hist2, ok, aug = _friction_reference(fraction)
    m, top, bottom, f, dofs = _seat(kind, rollers="y")
    X = np.asarray(m.vertices)
    obstacles = ts._fa_obstacles(FRICTION_OBS, [FRICTION_MU, 0.0], slip_length=FRICTION_EPS)
    u0 = _friction_guesses(m, None, fraction)
    newton = _solver(engine, kind, op, obstacles, f, dofs).with_friction_reference(u0)
    al = fa.AugmentedLagrangian(newton, 30, AL_TOL)
    settings = fa.NewtonSettings(60, NEWTON_TOLERANCE)
    u = u0.copy()
    al.solve(u, settings, **NEWTON_KW)
    u1 = u.copy()
    con = fa.Contact(engine)
    s1 = con.multipliers()
    newton.with_friction_reference(u1).with_load(f + _side_load(m, fraction))
    assert np.array_equal(con.multipliers(), s1)             # (the lag state moves, the multipliers stay: a warm start)
    u = _friction_guesses(m, u1, fraction)
    res = al.solve(u, settings, **NEWTON_KW)
    R, Q = con.resultants()
    slip = (u - u1).reshape(-1, 3)[bottom, 0]
    print(f"fraction {fraction}: {res.updates} updates; slip {slip.min():.3e} .. {slip.max():.3e}; |Q| {np.linalg.norm(Q[0]):.4f} "
          f"mu |R| {FRICTION_MU * np.linalg.norm(R[0]):.4f}")
    # (the last update moved every multiplier by at most AL_TOL, and with it each node's force by at most k AL_TOL)
    bar = 10.0 * np.sqrt(X.size) * NEWTON_TOLERANCE + SEAT_K * len(bottom) * AL_TOL
    print(f"u against the reference loop: {_rel(u, u2_ref):.3e}")
    assert abs(R[0][2] + SEAT_F) <= bar
    if fraction < 1.0:
        assert np.abs(slip).max() < FRICTION_EPS and abs(Q[0][0] - fraction * FRICTION_MU * SEAT_F) <= FRICTION_MU * bar
    else:
        assert slip.min() > FRICTION_EPS
        assert abs(np.linalg.norm(Q[0]) - FRICTION_MU * np.linalg.norm(R[0])) <= 0.05 * FRICTION_MU * np.linalg.norm(R[0])


# ------------------------------------------------------------------------------------------ 11: a frozen field in time
def _frozen_scene(kind, bottom=0.03, mid=0.51):
    """the drop of test_contact (v_0 = (0, 0, -1) over the floor z >= -0.02) with multipliers standing on the bottom face (`bottom`) and the
    one above (`mid`): the floor acts that far above itself there, so the cube meets it before its nodes reach z = -0.02"""
    m = tc._mesh(kind)[0]
    X = np.asarray(m.vertices)
    s = np.zeros((1, len(X)))
    s[0, tc._face(m, 2, 0.0)] = bottom
    s[0, tc._face(m, 2, 0.5)] = mid
    return m, s


@pytest.mark.gpu
@pytest.mark.parametrize("kind,op", [("HEX8", "neo_hookean"), ("TET4", "elastic")])
def test_central_differences_with_multipliers_standing(engine, oracle, kind, op):
    """8 steps against dr.central_difference on the shifted law at the bar of test_dropped_cube_central_differences; 8 = 4 + 4 bit for bit"""
    m, s = _frozen_scene(kind)
    dt = tc._drop_dt(kind, op)[0]
    u0, v0 = tc._drop_state(m)

    def reference(perm):
        return dr.central_difference(ar.AugmentedProblem(tc._problem(oracle, kind, op, tc.FLOOR, perm=perm), s), u0, v0, dt, 8, 4)

    ref = reference(None)
    plain = dr.central_difference(tc._problem(oracle, kind, op, tc.FLOOR), u0, v0, dt, 8, 4)
    assert _rel(plain[0], ref[0]) > 1e-3                   # the multipliers act from the first step
    bound = max(20.0 * tc._traj_rel(reference(7), ref), 1e-13)

    def run(chunks):
        asm = tc._assembler(engine, kind, op)
        ti = fa.CentralDifference(asm, RHO, dt).with_obstacles(tc._fa_obstacles(tc.FLOOR))
        fa.Contact(engine).set_multipliers(s)
        ti.set_state(u0, v0)
        rows = [tc._records(ti.step(c, 4)) for c in chunks]
        u, v, a, _, step = ti.state()
        assert step == 8 and np.array_equal(fa.Contact(engine).multipliers(), s)      # frozen: no route updates them
        ti.close()
        return u, v, a, np.concatenate(rows)

    got = run([8])
    _check("trajectory", tc._traj_rel(got, ref), bound)
    again = run([4, 4])
    for p, q in zip(got, again):
        assert np.array_equal(p, q)


@pytest.mark.gpu
def test_newmark_with_multipliers_standing(engine, oracle):
    """2 Newmark steps against dr.implicit on the shifted law at the bar of test_dropped_cube_implicit"""
    kind, op = "HEX8", "neo_hookean"
    # (the bottom face 0.002 inside the shifted floor at the start, the mid layer 0.005 above it: it joins in the first step)
    m, s = _frozen_scene(kind, 0.022, 0.515)
    dt = 8.0 * tc._drop_dt(kind, op)[0]
    u0, v0 = tc._drop_state(m)
    tol = 1e-10

    def reference(perm, t):
        st, u, v, a, rec, done, _ = dr.implicit(ar.AugmentedProblem(tc._problem(oracle, kind, op, tc.FLOOR, perm=perm), s), "newmark", u0, v0, dt, 2, 1, tol=t)
        assert st == "ok" and done == 2
        return u, v, a, rec

    ref = reference(None, tol)
    plain = dr.implicit(tc._problem(oracle, kind, op, tc.FLOOR), "newmark", u0, v0, dt, 2, 1, tol=tol)
    assert _rel(plain[1], ref[0]) > 1e-3 and ((cr.phi_table(tc.FLOOR, m.vertices, ref[0]) - s) < 0).any()
    bound = max(20.0 * (tc._traj_rel(reference(7, tol), ref) + tc._traj_rel(reference(None, tol / 100.0), ref)), 1e-13)
    asm = tc._assembler(engine, kind, op)
    ti = fa.Newmark(asm, RHO, dt).with_newton(fa.NewtonSettings(40, tol), linear_rel_tol=1e-13).with_obstacles(tc._fa_obstacles(tc.FLOOR))
    fa.Contact(engine).set_multipliers(s)
    ti.set_state(u0, v0)
    rec = ti.step(2, 1)
    u, v, a, _, _ = ti.state()
    ti.close()
    _check("newmark", tc._traj_rel((u, v, a, tc._records(rec)), ref), bound)


@pytest.mark.gpu
def test_stable_dt_sees_the_enlarged_active_set(engine, oracle):
    """fh_dynamics_stable_dt at u = 0 over the floor z >= -0.02: nothing touches it, omega_max is the free body's; with multipliers on the
    bottom face those nodes are active and omega_max^2 is dr.power_iteration's on the shifted law, several times larger"""
    kind, op = "HEX8", "neo_hookean"
    m, s = _frozen_scene(kind)
    prob = tc._problem(oracle, kind, op, tc.FLOOR)
    u = np.zeros(prob.n)
    rq, rq_free = dr.power_iteration(ar.AugmentedProblem(prob, s), u, 40), dr.power_iteration(prob, u, 40)
    rq_perm = dr.power_iteration(ar.AugmentedProblem(tc._problem(oracle, kind, op, tc.FLOOR, perm=7), s), u, 40)
    bound = max(20.0 * abs(rq_perm - rq) / rq, 1e-13)
    assert rq > 2.0 * rq_free
    asm = tc._assembler(engine, kind, op)
    ti = fa.CentralDifference(asm, RHO, 1e-3).with_obstacles(tc._fa_obstacles(tc.FLOOR))
    ti.set_state(u)
    om_free, _ = ti.stable_dt(40)
    fa.Contact(engine).set_multipliers(s)
    om, dtc = ti.stable_dt(40)
    ti.close()
    print(f"omega_max^2: reference {rq:.1f} (no multipliers {rq_free:.1f}), device {om * om:.1f} ({om_free ** 2:.1f})")
    _check("omega_max^2", abs(om * om - rq) / rq, bound)
    _check("omega_max^2 without", abs(om_free ** 2 - rq_free) / rq_free, bound)
    assert dtc == 2.0 / om


# ------------------------------------------------------------------------------------------ 12: argument errors and lifetimes
@pytest.mark.gpu
def test_multiplier_argument_errors_and_lifetimes(engine):
    import ctypes as C

    lib, h = engine._lib, engine._h
    floor = fa.HalfSpace((0, 0, 0.1), (0, 0, 1), 1e3, path=fa.ObstaclePath([0.0, 1.0], [[0, 0, 0], [0, 0, 0.1]]))
    asm = tc._assembler(engine, "HEX8", "elastic")
    N = engine.num_nodes()
    con = fa.Contact(engine)
    s = np.random.default_rng(3).uniform(0.0, 0.1, (1, N))
    st = _ffi.MultiplierUpdateStats()
    out = np.zeros(N)
    # no obstacles
    assert lib.fh_set_contact_multipliers(h, _ffi.fp(s.ravel())) == FH_INVALID_STATE
    assert lib.fh_contact_multipliers(h, _ffi.fp(out)) == FH_INVALID_STATE
    assert lib.fh_contact_multiplier_update(h, None, 0, C.byref(st)) == FH_INVALID_STATE
    assert lib.fh_set_contact_multipliers(h, None) == 0                    # clearing needs none
    engine.set_obstacles([floor])
    assert not con.multipliers().any() and not con.multiplier_forces().any()          # zeros while none are set
    for bad in (-1e-3, np.nan, np.inf):
        t = s.copy()
        t[0, 5] = bad
        assert _code(con.set_multipliers, t) == FH_BAD_ARGUMENT
        assert not con.multipliers().any()                                # a failed call leaves them as they were
    with pytest.raises(ValueError):
        con.set_multipliers(np.zeros(N + 1))
    assert lib.fh_contact_multipliers(h, None) == FH_BAD_ARGUMENT and lib.fh_contact_multiplier_forces_dev(h, None) == FH_BAD_ARGUMENT
    skip = np.array([N], dtype=np.uint64)
    assert lib.fh_contact_multiplier_update(h, _ffi.up(skip), 1, C.byref(st)) == FH_BAD_ARGUMENT
    assert lib.fh_contact_multiplier_update(h, None, 1, C.byref(st)) == FH_BAD_ARGUMENT
    con.set_multipliers(s)
    assert np.array_equal(con.multipliers(), s)
    _check("forces", _rel(con.multiplier_forces(), 1e3 * s), SHORT_SUM)
    # kept by the clock, by friction and by a new u; cleared by the obstacle list and by the mesh
    engine.set_obstacle_time(0.5, 0.25)
    assert np.array_equal(con.multipliers(), s)
    engine._check(lib.fh_set_friction(h, _ffi.fp(np.array([0.3])), 1, 1e-3))
    engine._check(lib.fh_set_friction_reference(h, None))
    assert np.array_equal(con.multipliers(), s)
    asm.with_u(np.full(3 * N, -0.01))
    assert np.array_equal(con.multipliers(), s)
    engine.set_obstacles([floor])
    assert not con.multipliers().any()
    # the first update allocates zeros: s = the penetration; skip nodes are honoured; stats may be NULL
    asm.with_u(np.full(3 * N, -0.2))
    up = con.update_multipliers([0, 1])
    got = con.multipliers()[0]
    X = np.asarray(tc._mesh("HEX8")[0].vertices)
    want = np.maximum(0.0, -(X[:, 2] - 0.2 - 0.1))
    want[[0, 1]] = 0.0
    assert np.array_equal(got, want) and up.active == (want > 0).sum() and up.max_change == want.max()
    assert up.max_penetration == want.max() and up.max_force == 1e3 * want.max()
    assert lib.fh_contact_multiplier_update(h, None, 0, None) == 0
    assert np.array_equal(con.multipliers()[0], want + np.maximum(0.0, -(X[:, 2] - 0.2 - 0.1)))
    asm = tc._assembler(engine, "HEX8", "elastic")             # fh_set_mesh: the obstacles go, and the multipliers with them
    assert lib.fh_contact_multipliers(h, _ffi.fp(out)) == FH_INVALID_STATE
    engine.set_obstacles([floor])
    assert not con.multipliers().any()
    # the outer loop: its errors
    newton = fa.MatrixFreeNewton(asm)
    with pytest.raises(ValueError):
        fa.AugmentedLagrangian(newton).solve(np.zeros(3 * N))
    bottom = tc._face(tc._mesh("HEX8")[0], 2, 0.0)
    f = np.zeros(3 * N)
    f[2::3] = -0.1
    newton = fa.MatrixFreeNewton(asm).with_dirichlet_dofs(tc._face(tc._mesh("HEX8")[0], 0, 0.0), [0]).with_dirichlet_dofs(
        tc._face(tc._mesh("HEX8")[0], 1, 0.0), [1]).with_load(f).with_obstacles(fa.Obstacles([fa.HalfSpace((0, 0, 0), (0, 0, 1), 1e2)]))
    guess = np.zeros(3 * N)
    guess[2::3] = f[2::3].sum() / (1e2 * len(bottom))          # (at u = 0 the bottom nodes are ON the floor: nothing would hold the block)
    with pytest.raises(fa.AugmentedLagrangianError) as e:
        fa.AugmentedLagrangian(newton, max_updates=2, tol=1e-14).solve(guess, fa.NewtonSettings(40, 1e-10), **NEWTON_KW)
    assert e.value.result.updates == 2 and not e.value.result.converged and len(e.value.result.multiplier_updates) == 2


@pytest.mark.gpu
def test_multipliers_travel_with_their_owner(engine):
    """another object uses the engine in between: bind_obstacles hands the obstacles over again, and the multipliers with them"""
    kind, op = "HEX8", "neo_hookean"
    m = tc._mesh(kind)[0]
    X = np.asarray(m.vertices)
    u = tc._random_u(m)
    obs = tc._three_kinds(3)
    s = _random_s(obs, X, u)
    asm = tc._assembler(engine, kind, op, u)
    x = np.random.default_rng(6).uniform(-1.0, 1.0, X.size)
    t = fa.MatrixFreeTangent(asm).with_obstacles(tc._fa_obstacles(obs))
    fa.Contact(engine).set_multipliers(s)
    y = t.apply(np.zeros_like(x), x).copy()
    other = fa.MatrixFreeTangent(asm)                       # owns no obstacles: clears them from the engine
    y_other = other.apply(np.zeros_like(x), x).copy()
    assert fa.Contact(engine)._count() == 0
    assert np.array_equal(t.apply(np.zeros_like(x), x), y) and not np.array_equal(y, y_other)
    assert np.array_equal(fa.Contact(engine).multipliers(), s)
    t.with_obstacles(tc._fa_obstacles(obs))                  # new obstacles: no multipliers
    assert not fa.Contact(engine).multipliers().any()
