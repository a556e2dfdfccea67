"""Coulomb friction on the penalty contact (fh_set_friction, fh_friction_*, fh_dynamics_set_slip_velocity, fenris_amd.contact) against the
NumPy statement of tests/friction_reference.py, which is pinned here on the CPU against central differences of its own potential and force.

Bounds.  The term itself is a short sum per node: 1e-13 of the largest entry, as in test_contact.py.  Where the term rides on a Newton solve
or a trajectory the bound is 1e-13 as well, and where that is exceeded it is measured from the reference alone and printed: d_ld, the
float64 run of the reference against its np.longdouble run, times 8:  bound = max(8 d_ld, 1e-13).  For LinearElastic the long-double run
is friction_reference.LongDoubleElastic, where the elastic residual, the mass, the contact force, the friction term, the integrator and
Newton's iterates are all np.longdouble (pinned below against the oracle's matrices); for StableNeoHookean the element terms come from
stable_neo_hookean_reference, which forms them in np.longdouble in either run, and the friction term is switched.  MEASURED records what
the CPU gave."""
import functools
import os

import numpy as np
import pytest

import fenris_amd as fa
from fenris_amd import _ffi, quadrature

import contact_reference as cr
import dynamics_reference as dr
import friction_reference as fr

LAME = fa.LameParameters(384.0, 577.0)
RHO = 1.0
FH_BAD_ARGUMENT, FH_INVALID_STATE, FH_UNSUPPORTED = 2, 5, 6
OKIND = {"QUAD4": 0, "HEX8": 1, "TET4": 2, "HEX27": 3, "TET10": 5}
NEW = ("fh_set_friction", "fh_set_friction_reference", "fh_set_friction_reference_dev", "fh_friction_potential", "fh_friction_force_dev",
       "fh_dynamics_set_slip_velocity")
SHORT_SUM = 1e-13
EPS = 2.0 ** -7

# measured on the CPU with the reference alone: (d_ld, bound); the tests measure them again and print them
MEASURED = {"stick elastic": (6.8e-15, 1.0e-13), "stick stable": (8.2e-17, 1.0e-13),
            "slide central u, v, a": ((6.5e-16, 1.0e-13), (2.4e-15, 1.0e-13), (9.9e-14, 8.0e-13)),
            "slide newmark u, v, a": ((1.0e-14, 1.0e-13), (7.1e-14, 5.7e-13), (1.5e-12, 1.2e-11)),
            "slide euler u, v, a": ((3.6e-15, 1.0e-13), (2.1e-14, 1.7e-13), (5.3e-13, 4.2e-12))}


@pytest.fixture()
def engine():
    eng = fa.Engine(0)
    yield eng
    eng.close()


# ------------------------------------------------------------------------------------------ meshes, obstacles, the scene of the term tests
@functools.lru_cache(maxsize=None)
def _mesh(kind):
    P, T, Q = fa.procedural, quadrature.tensor, quadrature.total_order
    make = {"HEX8_3": (lambda: P.create_unit_box_uniform_hex_mesh_3d(3), T.hexahedron_gauss(2)),
            "HEX8_776": (lambda: P.create_rectangular_uniform_hex_mesh(1.0 / 7.0, 7, 7, 6, 1), T.hexahedron_gauss(2)),   # 294 elements: two tiles
            "HEX8_332": (lambda: P.create_rectangular_uniform_hex_mesh(1.0 / 3.0, 3, 3, 2, 1), T.hexahedron_gauss(2)),   # the block of the solves
            "QUAD4_4": (lambda: P.create_unit_square_uniform_quad_mesh_2d(4), T.quadrilateral_gauss(2)),
            "TET4": (lambda: P.create_unit_box_uniform_tet_mesh_3d(2), Q.tetrahedron(2)),
            "TET10": (lambda: fa.tet10_mesh_from_tet4(P.create_unit_box_uniform_tet_mesh_3d(2)), Q.tetrahedron(4)),
            "HEX27": (lambda: fa.hex27_mesh_from_hex8(P.create_unit_box_uniform_hex_mesh_3d(2)), T.hexahedron_gauss(3))}
    gen, (w, p) = make[kind]
    return gen(), np.asarray(w), np.asarray(p)


def _okind(kind):
    return OKIND[kind.split("_")[0]]


def _fa_obstacles(obstacles, mu=None, node_weights=None, **kw):
    out = []
    for j, (kind, p, q, k) in enumerate(obstacles):
        cls = fa.HalfSpace if kind == "half_space" else fa.Ball if kind == "ball" else fa.Cavity
        out.append(cls(p, q, k, friction=0.0 if mu is None else mu[j]))
    return fa.Obstacles(out, node_weights, **kw)


def _material(op):
    return {"elastic": fa.LinearElasticMaterial, "stable": fa.StableNeoHookeanMaterial}[op]()


def _lame(op, d=3):
    return LAME.for_stable_neo_hookean(d) if op == "stable" else LAME


def _assembler(engine, kind, op, u=None, qt=None):
    m, w, p = _mesh(kind)
    d = m.vertices.shape[1]
    if qt is None:
        qt = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(_lame(op, d))
    return (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(m).with_operator(fa.MaterialEllipticOperator(_material(op)))
            .with_quadrature_table(qt).with_u(np.zeros(m.vertices.size) if u is None else u).build())


def _rel(x, y):
    return np.abs(np.asarray(x) - np.asarray(y)).max() / max(np.abs(np.asarray(y)).max(), 1e-300)


def _check(name, err, tol):
    print(f"{name}: {err:.3e} (bound {tol:.3e})")
    assert err <= tol, (name, err, tol)


def _bound(d_ld):
    return max(8.0 * d_ld, 1e-13)


def _code(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except fa.FenrisError as e:
        return e.code
    return 0


@functools.lru_cache(maxsize=None)
def _scene(kind):
    """obstacles, coefficients, ubar, u, node weights and the named nodes of the term tests on the mesh `kind`, every case of the issue placed
    by construction.  The last axis is "up"; the floor x_up >= 0.3 has the normal e_up exactly, so a slip along axis 0 is exact."""
    X = np.asarray(_mesh(kind)[0].vertices)
    N, d = X.shape
    up = d - 1
    rng = np.random.default_rng(21)
    ubar = rng.uniform(-0.02, 0.02, (N, d))
    step = rng.uniform(-0.02, 0.02, (N, d))
    w = rng.uniform(0.5, 2.0, N)
    low = [int(i) for i in np.argsort(X[:, up], kind="stable") if X[i, up] < 0.28]
    assert len(low) >= 9, len(low)
    names = ("zero", "inside", "edge", "far", "enters", "leaves", "weightless", "fixed", "centre")
    node = dict(zip(names, low[:: max(1, len(low) // 9)][:9]))
    assert len(set(node.values())) == 9
    for name in names:   # an exact lag state under the floor: ubar = (2^-6, ..., 0)
        ubar[node[name]] = 2.0 ** -6
        ubar[node[name], up] = 0.0
        step[node[name]] = 0.0
    step[node["inside"], 0] = 0.3 * EPS
    step[node["edge"], 0] = EPS                # |s| == eps to the bit
    step[node["far"], 0] = 100.0 * EPS
    ubar[node["enters"], up] = 0.5             # out of contact at ubar, in contact at u
    step[node["enters"], up] = -0.5
    step[node["enters"], 0] = 0.5 * EPS
    step[node["leaves"], up] = 0.5             # in contact at ubar, out of contact at u
    step[node["leaves"], 0] = 2.0 * EPS
    step[node["weightless"], 0] = 2.0 * EPS
    w[node["weightless"]] = 0.0
    step[node["fixed"], 0] = 0.5 * EPS
    u = ubar + step
    point = np.zeros(d)
    point[up] = 0.3
    normal = np.zeros(d)
    normal[up] = 1.0
    centre = X[node["centre"]] + ubar[node["centre"]]      # a ball centred on a node's lag position: no gradient there
    obstacles = [("half_space", tuple(point), tuple(normal), 1.0e4), ("ball", tuple(centre), 0.4, 2.0e3),
                 ("cavity", (0.4, 0.5, 0.6)[:d], 0.75 if d == 3 else 0.6, 5.0e3), ("half_space", (0.3,) * d, (1.0, 2.0, 3.0)[:d], 1.0e4)]
    mu = [0.5, 0.3, 0.7, 0.2]
    return obstacles, mu, ubar.reshape(-1), u.reshape(-1), w, node


def _assert_scene(kind):
    """the cases the issue lists occur, as the reference sees them"""
    obs, mu, ubar, u, w, node = _scene(kind)
    X = np.asarray(_mesh(kind)[0].vertices)
    d = X.shape[1]
    floor = ([obs[0]], [mu[0]])
    slip = {}
    for i, ml, n, s, y in fr._visit(*floor, X, ubar, u - ubar, None, np.float64):
        slip[i] = float(y)
    assert slip[node["zero"]] == 0.0 and 0.0 < slip[node["inside"]] < EPS and slip[node["edge"]] == EPS and slip[node["far"]] == 100.0 * EPS
    phi_bar, phi_u = cr.phi_table([obs[0]], X, ubar)[0], cr.phi_table([obs[0]], X, u)[0]
    assert phi_bar[node["enters"]] > 0 > phi_u[node["enters"]] and node["enters"] not in slip
    assert phi_bar[node["leaves"]] < 0 < phi_u[node["leaves"]] and slip[node["leaves"]] > 0.0
    assert fr._eval(obs[1], (X + ubar.reshape(X.shape))[node["centre"]], np.float64) == (-0.4, None)
    both = [i for i in range(len(X)) if cr.phi_table([obs[0], obs[3]], X, ubar)[:, i].max() < 0]
    assert len(both) >= 1
    assert w[node["weightless"]] == 0.0 and phi_bar[node["fixed"]] < 0


# ------------------------------------------------------------------------------------------ no GPU: declarations, the reference pinned
def test_friction_entry_points_are_declared():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fenris_hip.h")).read()
    for name in NEW:
        assert name in _ffi.exported_symbols() and name + "(" in hdr
    for cls in (fa.MatrixFreeTangent, fa.MatrixFreeShiftedTangent, fa.MatrixFreeNewton):
        assert callable(getattr(cls, "with_friction_reference"))
    assert callable(fa.Contact.friction_potential) and callable(fa.Contact.friction_force)
    assert fa.HalfSpace((0, 0, 0), (0, 0, 1), 1.0).friction == 0.0 and fa.Ball((0, 0, 0), 1.0, 1.0, friction=0.25).friction == 0.25
    obs = fa.Obstacles([fa.Cavity((0, 0, 0), 1.0, 1.0, 0.5)], slip_velocity=0.1)
    assert obs.has_friction() and obs.slip_length_for(0.5) == 0.05
    with pytest.raises(ValueError):
        obs.slip_length_for(None)     # a solver has no dt: it needs a slip length
    with pytest.raises(ValueError):
        fa.Obstacles([fa.Cavity((0, 0, 0), 1.0, 1.0, 0.5)]).slip_length_for(0.5)
    assert not fa.Obstacles([fa.Cavity((0, 0, 0), 1.0, 1.0)]).has_friction()
    with pytest.raises(ValueError):
        fa.contact.with_friction_reference(object(), None)     # the lag displacement itself is asked for, and copied


def _fd_scene(d, seed):
    """a random cloud around the three kinds of obstacle, clear of the switches of the lag state"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.0, 1.0, (60 * d, d))
    obs = [("half_space", (0.3,) * d, (1.0, 2.0, 3.0)[:d], 1.0e4), ("ball", (1.1,) * d, 0.7, 2.0e3), ("cavity", (0.4, 0.5, 0.6)[:d], 0.75 if d == 3 else 0.6, 5.0e3)]
    ubar = rng.uniform(-0.02, 0.02, X.size)
    u = ubar + (rng.uniform(-0.02, 0.02, X.shape) * rng.choice([0.1, 1.0], (len(X), 1))).reshape(-1)     # slips on both sides of eps
    return X, obs, [0.5, 0.3, 0.7], ubar, u, rng.uniform(0.5, 2.0, len(X))


@pytest.mark.parametrize("d", [2, 3])
def test_reference_force_is_the_gradient_of_the_potential(d):
    """q against central differences of D, the three kinds, slips on both sides of eps"""
    X, obs, mu, ubar, u, w = _fd_scene(d, 1)
    ys = [float(y) for _, _, _, _, y in fr._visit(obs, mu, X, ubar, u - ubar, w, np.float64)]
    assert min(ys) < 0.5 * EPS and max(ys) > 2.0 * EPS and len(ys) >= 10
    for j in range(3):
        assert any(True for _ in fr._visit([obs[j]], [mu[j]], X, ubar, u - ubar, w, np.float64)), obs[j][0]
    q = fr.force(obs, mu, X, ubar, u - ubar, EPS, w)
    h = 1e-6
    fd = np.zeros_like(q)
    for i in range(len(u)):
        e = np.zeros_like(u)
        e[i] = h
        fd[i] = (fr.potential(obs, mu, X, ubar, u + e - ubar, EPS, w) - fr.potential(obs, mu, X, ubar, u - e - ubar, EPS, w)) / (2 * h)
    _check(f"{d}-D q vs dD", _rel(fd, q), 2e-8)
    lam_max = max(float(ml) for _, ml, _, _, _ in fr._visit(obs, mu, X, ubar, u - ubar, w, np.float64))
    assert np.abs(q).max() <= lam_max * (1 + 1e-12) * len(obs)      # |q_i| <= sum_o mu_o lam


@pytest.mark.parametrize("d", [2, 3])
def test_reference_block_is_the_derivative_of_the_force_and_psd(d):
    """H against central differences of q; H symmetric with smallest eigenvalue >= -1e-12 |H|"""
    X, obs, mu, ubar, u, w = _fd_scene(d, 2)
    H = fr.tangent(obs, mu, X, ubar, u - ubar, EPS, w).toarray()
    h = 1e-7
    fd = np.zeros_like(H)
    for i in range(len(u)):
        e = np.zeros_like(u)
        e[i] = h
        fd[:, i] = (fr.force(obs, mu, X, ubar, u + e - ubar, EPS, w) - fr.force(obs, mu, X, ubar, u - e - ubar, EPS, w)) / (2 * h)
    _check(f"{d}-D H vs dq", _rel(fd, H), 2e-7)
    B = fr.blocks(obs, mu, X, ubar, u - ubar, EPS, w)
    size = np.abs(B).max()
    assert np.abs(B - B.transpose(0, 2, 1)).max() <= 1e-12 * size
    assert min(np.linalg.eigvalsh(0.5 * (b + b.T)).min() for b in B) >= -1e-12 * size


@pytest.mark.parametrize("kind", ["HEX8_3", "QUAD4_4"])
def test_reference_special_nodes(kind):
    """the constructed cases: q = 0 at slip 0 with a block 2 mu lam / eps P; |q| = mu lam at and beyond eps; nothing at the ball's centre"""
    _assert_scene(kind)
    obs, mu, ubar, u, w, node = _scene(kind)
    X = np.asarray(_mesh(kind)[0].vertices)
    d = X.shape[1]
    floor, fmu = [obs[0]], [mu[0]]
    q = fr.force(floor, fmu, X, ubar, u - ubar, EPS, w).reshape(-1, d)
    H = fr.blocks(floor, fmu, X, ubar, u - ubar, EPS, w)
    lam = {i: float(ml) for i, ml, _, _, _ in fr._visit(floor, fmu, X, ubar, u - ubar, w, np.float64)}
    z = node["zero"]
    assert not q[z].any() and H[z][0, 0] == lam[z] * 2.0 / EPS and H[z][d - 1, d - 1] == 0.0
    for name in ("edge", "far"):
        assert abs(np.linalg.norm(q[node[name]]) - lam[node[name]]) <= 1e-15 * lam[node[name]]
        assert abs(H[node[name]][0, 0]) <= 1e-12 * lam[node[name]] / EPS      # no stiffness along a slip of eps or more
    assert not q[node["enters"]].any() and q[node["leaves"]].any() and not q[node["weightless"]].any()
    ball = fr.force([obs[1]], [mu[1]], X, ubar, u - ubar, EPS, w).reshape(-1, d)
    assert not ball[node["centre"]].any() and ball.any()
    assert not fr.force(obs, [0.0] * 4, X, ubar, u - ubar, EPS, w).any()


@pytest.mark.parametrize("kind", ["HEX8_332", "TET4"])
def test_long_double_reference_matches_the_oracle(oracle, kind):
    """LongDoubleElastic's stiffness and mass, rounded to double, are the oracle's assembled matrices, and its contact force is cr.force"""
    m, w, p = _mesh(kind)
    conn = np.asarray(m.connectivity)
    groups = [(conn, w, p)]
    if kind == "TET4":      # the two rules of the rule-set table
        w2, p2 = (np.asarray(a) for a in quadrature.total_order.tetrahedron(3))
        emap = np.arange(len(conn)) % 3 == 0
        groups = [(conn[~emap], w, p), (conn[emap], w2, p2)]
    floor = [("half_space", (0.0, 0.0, 0.1), (0.0, 0.0, 1.0), 1e3)]
    ld = fr.LongDoubleElastic(kind.split("_")[0], m.vertices, groups, LAME.mu, LAME.lambda_, RHO, None, floor)
    prob = cr.ContactProblem(oracle, _okind(kind), oracle.LINEAR_ELASTIC, m.vertices, groups, params=LAME.as_pair(), rho=RHO, obstacles=floor)
    u = _random_u_of(m)
    _check(f"{kind} K", _rel(ld.K.astype(np.float64), dr.Problem.tangent(prob, u).toarray()), 1e-13)
    _check(f"{kind} M", _rel(ld.M.astype(np.float64), prob.mass().toarray()), 1e-13)
    _check(f"{kind} r + g", _rel(ld.residual(u).astype(np.float64), prob.residual(u)), 1e-13)
    assert np.abs(prob.contact_force(u)).max() > 0.0


def _random_u_of(m):
    return np.random.default_rng(1).uniform(-0.02, 0.02, m.vertices.size)


# ------------------------------------------------------------------------------------------ GPU 1: the term itself
def _set(engine, obs, mu, w, ubar, eps=EPS):
    engine.set_obstacles(_fa_obstacles(obs, mu, w, slip_length=eps))
    engine._check(engine._lib.fh_set_friction_reference(engine._h, _ffi.fp(np.ascontiguousarray(ubar))))


def _csr_added(engine, asm):
    k = fa.CsrAssembler(fa.SCATTER_GATHER).assemble(asm)
    vals = np.zeros_like(k.values)
    fa.Contact(engine).add_tangent_to(vals)
    return fa.CsrMatrix(k.row_offsets, k.col_indices, vals).to_scipy().toarray()


def _rule_set_tet4():
    m, w, p = _mesh("TET4")
    w2, p2 = (np.asarray(a) for a in quadrature.total_order.tetrahedron(3))
    emap = (np.arange(m.num_elements()) % 3 == 0).astype(np.uint64)
    return fa.compact_quadrature_table([p, p2], [w, w2], [[LAME] * len(w), [LAME] * len(w2)], emap)


TERM_CASES = [("HEX8_3", "elastic", "uniform", "tiles"), ("HEX8_3", "stable", "uniform", "tiles"), ("QUAD4_4", "elastic", "uniform", "tiles"),
              ("HEX8_776", "elastic", "uniform", "tiles"), ("TET10", "elastic", "uniform", "off"), ("HEX27", "elastic", "uniform", "off"),
              ("TET4", "elastic", "rule_set", None)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,op,table,route", TERM_CASES)
def test_term_parity(engine, kind, op, table, route):
    """fh_friction_potential, fh_friction_force_dev, the CSR blocks and the tangent's map and diagonal with friction minus the same with
    mu = 0, against the reference on the constructed scene; with a Dirichlet node in contact the free rows still carry H x"""
    import torch

    _assert_scene(kind)
    obs, mu, ubar, u, w, node = _scene(kind)
    X = np.asarray(_mesh(kind)[0].vertices)
    N, d = X.shape
    n = X.size
    asm = _assembler(engine, kind, op, u, _rule_set_tet4() if table == "rule_set" else None)
    _set(engine, obs, mu, w, ubar)
    con = fa.Contact(engine)
    D_ref, q_ref = fr.potential(obs, mu, X, ubar, u - ubar, EPS, w), fr.force(obs, mu, X, ubar, u - ubar, EPS, w)
    H_ref = fr.tangent(obs, mu, X, ubar, u - ubar, EPS, w).toarray()
    B_ref = cr.tangent(obs, X, u, w, exact=False).toarray()
    _check(f"{kind} potential", abs(con.friction_potential() - D_ref) / D_ref, SHORT_SUM)
    assert engine.last_kernel_name() == "k_friction_potential"
    garbage = np.random.default_rng(5).uniform(-1.0, 1.0, n + 64)
    buf = torch.tensor(garbage, device="cuda:0")
    con.friction_force(device=True, out=buf[32:32 + n])        # ADDS q, and q alone
    got = buf.cpu().numpy()
    assert np.array_equal(got[:32], garbage[:32]) and np.array_equal(got[32 + n:], garbage[32 + n:])
    _check(f"{kind} force into garbage", np.abs(got[32:32 + n] - garbage[32:32 + n] - q_ref).max() / np.abs(q_ref).max(), SHORT_SUM + 2.3e-16)
    q = con.friction_force()
    _check(f"{kind} force", _rel(q, q_ref), SHORT_SUM)
    assert not q.reshape(N, d)[node["zero"]].any() and not q.reshape(N, d)[node["weightless"]].any()
    _check(f"{kind} contact force unchanged", _rel(con.force(), cr.force(obs, X, u, w)), SHORT_SUM)
    _check(f"{kind} csr blocks B + H", np.abs(_csr_added(engine, asm) - (B_ref + H_ref)).max() / np.abs(B_ref + H_ref).max(), SHORT_SUM)
    # the tangent's map and diagonal with friction minus the same with every mu = 0
    x = np.random.default_rng(6).uniform(-1.0, 1.0, n)
    for bc in (None, np.array([node["fixed"], node["far"]], dtype=np.int64)):
        t = fa.MatrixFreeTangent(asm).with_dirichlet_nodes(bc).with_obstacles(_fa_obstacles(obs, mu, w, slip_length=EPS)).with_friction_reference(ubar)
        y1 = t.apply(np.zeros(n), x).copy()
        name = engine.last_kernel_name()
        d1 = t.diagonal()
        t0 = fa.MatrixFreeTangent(asm).with_dirichlet_nodes(bc).with_obstacles(_fa_obstacles(obs, None, w))
        y0, d0 = t0.apply(np.zeros(n), x).copy(), t0.diagonal()
        assert engine.last_kernel_name() == "k_contact_diagonal"
        free = np.ones(n, dtype=bool)
        if bc is not None:
            free[(d * bc[:, None] + np.arange(d)).reshape(-1)] = False
        Hx = H_ref @ np.where(free, x, 0.0)
        scale = max(np.abs(Hx).max(), np.abs(y0).max())
        _check(f"{kind} apply difference, dirichlet {bc is not None}", np.abs((y1 - y0) - Hx)[free].max() / scale, SHORT_SUM)
        _check(f"{kind} diagonal difference", np.abs((d1 - d0) - H_ref.diagonal())[free].max() / np.abs(d1).max(), SHORT_SUM)
        if bc is not None:      # the rows of the Dirichlet nodes: scale x, the scale that of the diagonal with B and H
            _check(f"{kind} dirichlet rows", _rel(y1[~free], d1[~free] * x[~free]), SHORT_SUM)
        if route == "tiles":
            assert name.endswith("k_operator_from_partials") and "k_contact_apply" not in name, name
        elif route == "off":
            assert name.endswith("+ k_contact_apply"), name


@pytest.mark.gpu
def test_reference_is_the_current_u_by_default_and_zero_before(engine):
    """until fh_set_friction_reference is called the lag state is u = 0; NULL takes the context's u"""
    kind = "HEX8_3"
    obs, mu, ubar, u, w, node = _scene(kind)
    X = np.asarray(_mesh(kind)[0].vertices)
    _assembler(engine, kind, "elastic", u)
    engine.set_obstacles(_fa_obstacles(obs, mu, w, slip_length=EPS))
    con = fa.Contact(engine)
    zero = np.zeros_like(u)
    _check("lag state 0", _rel(con.friction_force(), fr.force(obs, mu, X, zero, u, EPS, w)), SHORT_SUM)
    engine._check(engine._lib.fh_set_friction_reference(engine._h, None))
    assert not con.friction_force().any()                   # ubar = u: no slip anywhere
    D0 = fr.potential(obs, mu, X, u, zero, EPS, w)           # ... and D = sum mu lam eps / 3
    _check("potential at no slip", abs(con.friction_potential() - D0) / D0, SHORT_SUM)


# ------------------------------------------------------------------------------------------ GPU 2: mu = 0 changes nothing
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["HEX8_3", "TET10"])
def test_zero_coefficients_change_no_bit(kind):
    """friction set with every mu = 0 and a random ubar: the routes of test_contact.py give the bits of the frictionless run"""
    obs, _, ubar, _, w, _ = _scene(kind)
    m = _mesh(kind)[0]
    n = m.vertices.size
    X = np.asarray(m.vertices)
    top = np.where(np.isclose(X[:, 2], 1.0))[0]
    x = np.random.default_rng(12).uniform(-1.0, 1.0, n)
    f = np.zeros(n)
    f[3 * top + 2] = -2.0
    u_small = 0.1 * np.random.default_rng(13).uniform(-0.02, 0.02, n)

    def run(friction):
        eng = fa.Engine(0)
        try:
            asm = _assembler(eng, kind, "elastic", u_small)
            eng.set_obstacles(_fa_obstacles(obs, None, w))

            def arm():
                if friction:
                    eng._check(eng._lib.fh_set_friction(eng._h, _ffi.fp(np.zeros(len(obs))), len(obs), 0.37 * EPS))
                    eng._check(eng._lib.fh_set_friction_reference(eng._h, _ffi.fp(np.ascontiguousarray(ubar))))

            arm()
            con = fa.Contact(eng)
            pieces = [np.array([con.energy(), con.friction_potential()]), con.force(), con.friction_force(), _csr_added(eng, asm)]
            t = fa.MatrixFreeTangent(asm).with_dirichlet_nodes(top)       # (owns no obstacles: the engine's stay)
            pieces += [t.apply(np.zeros(n), x).copy(), t.diagonal()]
            s = fa.MatrixFreeShiftedTangent(asm, RHO, 1.0, 0.37).with_dirichlet_nodes(top)
            pieces += [s.apply(np.zeros(n), x).copy(), s.diagonal()]
            sol = np.zeros(n)
            pieces += [np.array([t.cg_solve(np.where(np.isin(np.arange(n) // 3, top), 0.0, x), sol, rel_tol=1e-8)]), sol]
            uu = np.array(u_small)     # (the scene is rough: the six iterations it gets, converged or not, must be the same six)
            solver = fa.MatrixFreeNewton(asm).with_dirichlet_nodes(top).with_load(f)
            pieces += [np.array([_code(solver.solve, uu, fa.NewtonSettings(6, 1e-9), linear_rel_tol=1e-10)]), uu]
            arm()
            if kind == "TET10":   # (no positive row-sum lumping on Tet10: backward Euler and Newmark instead)
                tis = [fa.BackwardEuler(asm, RHO, 1e-2), fa.Newmark(asm, RHO, 1e-2)]
                for ti in tis:
                    ti.with_newton(fa.NewtonSettings(6, 1e-9), linear_rel_tol=1e-10)
            else:
                tis = [fa.CentralDifference(asm, RHO, 1e-3), fa.BackwardEuler(asm, RHO, 1e-2).with_newton(fa.NewtonSettings(6, 1e-9), linear_rel_tol=1e-10)]
            for ti in tis:
                ti.with_dirichlet_nodes(top).with_load(f)
                ti.set_state(u_small, 0.01 * x)
                arm()
                if friction:
                    eng._check(eng._lib.fh_dynamics_set_slip_velocity(ti._handle(), 0.2))
                pieces += [np.array([_code(ti.step, 2 if not isinstance(ti, fa.CentralDifference) else 8, 4)])] + list(ti.state()[:3])
                ti.close()
            return pieces
        finally:
            eng.close()

    plain, armed = run(False), run(True)
    assert len(plain) == len(armed)
    for i, (p, q) in enumerate(zip(plain, armed)):
        assert np.array_equal(p, q), i


# ------------------------------------------------------------------------------------------ GPU 3: the stick test
BLOCK = "HEX8_332"
STICK_MU, STICK_EPS, STICK_K, STICK_P = 0.5, 1.0e-3, 1.0e4, 0.2
NEWTON_TOLERANCE = 1e-11
FLOOR = [("half_space", (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), STICK_K)]


def _problem(oracle, op, obstacles, f=None, rho=RHO, dtype=np.float64):
    """the reference's problem on the block; dtype np.longdouble: the LinearElastic problem in extended precision throughout"""
    m, w, p = _mesh(BLOCK)
    conn = np.asarray(m.connectivity)
    if op == "stable":
        return fr.StableProblem("HEX8", m.vertices, conn, w, p, _lame("stable"), rho, f, obstacles)
    if dtype is np.longdouble:
        return fr.LongDoubleElastic("HEX8", m.vertices, [(conn, w, p)], LAME.mu, LAME.lambda_, rho, f, obstacles)
    return cr.ContactProblem(oracle, OKIND["HEX8"], oracle.LINEAR_ELASTIC, m.vertices, [(conn, w, p)], params=LAME.as_pair(), rho=rho, f=f,
                             obstacles=obstacles)


def _stick_loads():
    X = np.asarray(_mesh(BLOCK)[0].vertices)
    top = np.where(np.isclose(X[:, 2], X[:, 2].max()))[0]
    bottom = np.where(np.isclose(X[:, 2], 0.0))[0]
    press = np.zeros(X.size)
    press[3 * top + 2] = -STICK_P
    shear = np.array(press)
    shear[3 * top] = 0.5 * STICK_MU * STICK_P        # half of mu times the normal load
    u0 = np.zeros(X.size)
    u0[2::3] = -STICK_P * len(top) / (STICK_K * len(bottom))     # the uniform penetration that carries the normal load
    return top, bottom, press, shear, u0


def _stick_reference(oracle, op, tol=NEWTON_TOLERANCE, dtype=np.float64):
    """press (lag state: the uniform penetration), move the lag state to the pressed u, shear: (u_pressed, u, FrictionProblem)"""
    top, bottom, press, shear, u0 = _stick_loads()
    fp = fr.FrictionProblem(_problem(oracle, op, FLOOR, dtype=dtype), [STICK_MU], STICK_EPS, u0, dtype)
    st, u1, _ = fr.newton(fp, u0, press, tol)
    assert st == "ok"
    fp.ubar = np.array(u1)
    st, u2, it = fr.newton(fp, u1, shear, tol)
    assert st == "ok"
    return u1, u2, fp


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["elastic", "stable"])
def test_newton_stick(engine, oracle, op):
    """a 3 x 3 x 2 block pressed onto the floor z >= 0 by a load on its top and sheared by half of mu times that load, no Dirichlet node:
    Newton converges, every bottom node sticks (slip < eps), the friction forces sum to the shear load, and u is the reference's"""
    top, bottom, press, shear, u0 = _stick_loads()
    u1_ref, u_ref, fp = _stick_reference(oracle, op)
    d_ld = _rel(np.asarray(_stick_reference(oracle, op, dtype=np.longdouble)[1], dtype=np.float64), u_ref)
    bound = _bound(d_ld)
    print(f"stick {op}: d_ld {d_ld:.2e} bound {bound:.2e}")
    slip_ref = fp.slip(u_ref)[bottom]
    assert 0.0 < slip_ref.max() < STICK_EPS, slip_ref.max()
    q_ref = fp.friction_force(u_ref).reshape(-1, 3)
    assert abs(q_ref[:, 0].sum() - shear[0::3].sum()) <= 1e-9 * abs(shear[0::3].sum())

    asm = _assembler(engine, BLOCK, op)
    obstacles = _fa_obstacles(FLOOR, [STICK_MU], slip_length=STICK_EPS)
    newton = fa.MatrixFreeNewton(asm).with_obstacles(obstacles).with_friction_reference(u0).with_load(press)
    settings = fa.NewtonSettings(40, NEWTON_TOLERANCE)
    u1 = np.array(u0)
    newton.solve(u1, settings, line_search=fa.BacktrackingLineSearch(), preconditioner=_ffi.PRECOND_JACOBI, linear_rel_tol=1e-13)
    _check("pressed", _rel(u1, u1_ref), bound)
    u = np.array(u1)
    res = newton.with_friction_reference(u1).with_load(shear).solve(u, settings, line_search=fa.BacktrackingLineSearch(),
                                                                     preconditioner=_ffi.PRECOND_JACOBI, linear_rel_tol=1e-13)
    print(f"sheared: {res.iterations} Newton iterations, |F| {res.residual_norm:.2e}; largest slip {slip_ref.max():.3e} of eps {STICK_EPS:.1e}")
    assert res.residual_norm <= NEWTON_TOLERANCE
    _check("sheared", _rel(u, u_ref), bound)
    fp.ubar = u1
    assert fp.slip(u)[bottom].max() < STICK_EPS
    q = fa.Contact(engine).friction_force().reshape(-1, 3)
    assert abs(q[:, 0].sum() - shear[0::3].sum()) <= 10.0 * NEWTON_TOLERANCE + 1e-13 * abs(shear[0::3].sum())
    assert abs(q[:, 1].sum()) <= 10.0 * NEWTON_TOLERANCE and not q[:, 2].any()


# ------------------------------------------------------------------------------------------ GPU 4: the slide test
# k, dt and eps_v chosen on the CPU so that the reference alone meets the 5 %: the friction that sets in at t = 0 rocks the block, and over the
# 0.032 time units of 64 steps the mean normal force is 2 to 3 % under the weight (k = 1e3, dt = 1e-3 gave 4 to 6 % over it)
SLIDE_MU, SLIDE_G, SLIDE_K, SLIDE_DT, SLIDE_EPS_V, SLIDE_V0, SLIDE_STEPS = 0.5, 10.0, 4.0e3, 5.0e-4, 0.05, 1.0, 64
# |F| <= 1e-14 in the implicit steps: a_{n+1} = (u_{n+1} - u_ref) / (beta dt^2) magnifies what the tolerance leaves in u by 1.6e7, and at
# 1e-10 the reference under a tolerance 100 times smaller differs by 1e-4 in a; at 1e-14 it does not differ (the rounding floor of |F| in this
# scene is some 1e-24)
SLIDE_TOL = 1e-14
SLIDE_FLOOR = [("half_space", (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), SLIDE_K)]


@functools.lru_cache(maxsize=None)
def _slide_state():
    """the block settled on the floor under gravity (the reference's Newton, friction holding it sideways), moving sideways at v_0"""
    from oracle import oracle as o

    o.lib()
    prob = _problem(o, "elastic", SLIDE_FLOOR)
    m = prob.lumped()
    f = np.zeros(prob.n)
    f[2::3] = -SLIDE_G * m[2::3]
    guess = np.zeros(prob.n)
    guess[2::3] = -SLIDE_G * m[2::3].sum() / (SLIDE_K * 16)
    fp = fr.FrictionProblem(prob, [SLIDE_MU], 1e-3, guess)
    st, u0, _ = fr.newton(fp, guess, f, 1e-12)
    assert st == "ok"
    v0 = np.zeros(prob.n)
    v0[0::3] = SLIDE_V0
    return u0, v0, f, m


def _slide_reference(oracle, scheme, tol=SLIDE_TOL, dtype=np.float64):
    u0, v0, f, _ = _slide_state()
    fp = fr.FrictionProblem(_problem(oracle, "elastic", SLIDE_FLOOR, f=f, dtype=dtype), [SLIDE_MU], None, None, dtype)
    if scheme == "central":
        return fr.central_difference(fp, u0, v0, SLIDE_DT, SLIDE_STEPS, SLIDE_EPS_V)
    out = fr.implicit(fp, scheme, u0, v0, SLIDE_DT, SLIDE_STEPS, SLIDE_EPS_V, tol=tol)
    assert out[0] == "ok"
    return out[1:]


def _deceleration(v_end):
    """the mean deceleration of the centre of mass over the run, from its momentum"""
    _, v0, _, m = _slide_state()
    return float((m[0::3] * (v0[0::3] - v_end[0::3])).sum() / m[0::3].sum()) / (SLIDE_STEPS * SLIDE_DT)


@pytest.mark.parametrize("scheme", ["central", "newmark", "euler"])
def test_reference_slide_decelerates_at_mu_g(oracle, scheme):
    """the scene is what the issue describes: the reference alone slides the whole run and loses mu g of speed per unit time within 5 %"""
    u, v, a, traj = _slide_reference(oracle, scheme)
    dec = _deceleration(v)
    print(f"{scheme}: deceleration {dec:.4f} against mu g = {SLIDE_MU * SLIDE_G}; slowest bottom node {v[0::3].min():.3f}")
    assert v[0::3].min() > 10.0 * SLIDE_EPS_V              # still sliding at the end
    assert abs(dec - SLIDE_MU * SLIDE_G) <= 0.05 * SLIDE_MU * SLIDE_G


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["central", "newmark", "euler"])
def test_slide(engine, oracle, scheme):
    """64 steps of the settled block sliding at v_0 = 1 on the floor with mu = 0.5: the trajectory is the reference integrator's, the run
    repeats bit for bit cut as 64, 32 + 32 and 8 x 8, and the centre of mass loses mu g of speed per unit time within 5 %"""
    u0, v0, f, m = _slide_state()
    tol = SLIDE_TOL
    ref = _slide_reference(oracle, scheme, tol=tol)
    # u, v and a round differently (a_{n+1} divides a difference of displacements by dt or dt^2): one measured bound each
    d_ld = [_rel(np.asarray(p, dtype=np.float64), q) for p, q in zip(_slide_reference(oracle, scheme, tol=tol, dtype=np.longdouble)[:3], ref[:3])]
    bound = [_bound(d) for d in d_ld]
    print(f"slide {scheme}: d_ld (u, v, a) {d_ld[0]:.2e} {d_ld[1]:.2e} {d_ld[2]:.2e}")
    obstacles = _fa_obstacles(SLIDE_FLOOR, [SLIDE_MU], slip_velocity=SLIDE_EPS_V)

    def run(chunks):
        asm = _assembler(engine, BLOCK, "elastic")
        ti = {"central": fa.CentralDifference, "newmark": fa.Newmark, "euler": fa.BackwardEuler}[scheme](asm, RHO, SLIDE_DT)
        if scheme != "central":
            ti.with_newton(fa.NewtonSettings(40, tol), linear_rel_tol=1e-13)
        ti.with_load(f).with_obstacles(obstacles)
        ti.set_state(u0, v0)
        for c in chunks:
            ti.step(c, 8)
        u, v, a, _, step = ti.state()
        assert step == SLIDE_STEPS
        ti.close()
        return u, v, a

    got = run([SLIDE_STEPS])
    for what, p, q, b in zip("uva", got[:3], ref[:3], bound):
        _check(f"slide {scheme} {what}", _rel(p, q), b)
    dec = _deceleration(got[1])
    print(f"deceleration {dec:.4f} against mu g = {SLIDE_MU * SLIDE_G}")
    assert abs(dec - SLIDE_MU * SLIDE_G) <= 0.05 * SLIDE_MU * SLIDE_G
    for chunks in ([32, 32], [8] * 8):
        again = run(chunks)
        for p, q in zip(got[:3], again[:3]):
            assert np.array_equal(p, q), chunks


# ------------------------------------------------------------------------------------------ GPU 5: refusals, arguments, launches
@pytest.mark.gpu
def test_set_friction_argument_errors(engine):
    lib, h = engine._lib, engine._h
    floor = fa.HalfSpace((0, 0, 0), (0, 0, 1), 1e3)
    one, two = _ffi.fp(np.array([0.5])), _ffi.fp(np.array([0.5, 0.5]))
    code = lambda rc: _code(engine._check, rc)
    asm = _assembler(engine, "HEX8_3", "elastic")
    assert code(lib.fh_set_friction(h, one, 1, 1e-3)) == FH_INVALID_STATE           # no obstacles
    assert code(lib.fh_set_friction(h, None, 0, 1e-3)) == 0                          # turning it off needs none
    assert code(lib.fh_set_friction_reference(h, None)) == FH_INVALID_STATE         # no friction set
    engine.set_obstacles([floor])
    assert code(lib.fh_set_friction(h, two, 2, 1e-3)) == FH_BAD_ARGUMENT            # count mismatch
    for bad in (-0.5, np.nan, np.inf):
        assert code(lib.fh_set_friction(h, _ffi.fp(np.array([bad])), 1, 1e-3)) == FH_BAD_ARGUMENT
    for bad in (0.0, -1e-3, np.nan, np.inf):
        assert code(lib.fh_set_friction(h, one, 1, bad)) == FH_BAD_ARGUMENT
    n = 3 * engine.num_nodes()
    asm.with_u(np.full(n, -0.01))
    con = fa.Contact(engine)
    assert con.friction_potential() == 0.0 and not con.friction_force().any()        # a failed call leaves friction off
    assert code(lib.fh_set_friction(h, one, 1, 1e-3)) == 0
    assert con.friction_potential() == 0.0                                           # the lag state u = 0 touches the floor nowhere
    assert code(lib.fh_set_friction_reference(h, None)) == 0                         # ... the current u does
    assert con.friction_potential() > 0.0 and not con.friction_force().any()
    shifted = np.full(n, -0.01)
    shifted[0::3] = 0.02
    asm.with_u(shifted)
    assert con.friction_force().any()
    assert code(lib.fh_set_friction(h, None, 0, 1e-3)) == 0                          # off again
    assert con.friction_potential() == 0.0
    assert code(lib.fh_set_friction(h, one, 1, 1e-3)) == 0
    engine.set_obstacles([floor])                                                    # fh_set_obstacles clears friction
    assert con.friction_potential() == 0.0 and not con.friction_force().any() and con.energy() > 0.0
    assert code(lib.fh_set_friction_reference(h, None)) == FH_INVALID_STATE
    # Python: friction without a length that fits the user
    with pytest.raises(ValueError):
        engine.set_obstacles(fa.Obstacles([fa.HalfSpace((0, 0, 0), (0, 0, 1), 1e3, friction=0.5)]))
    with pytest.raises(ValueError):
        fa.MatrixFreeNewton(asm).with_obstacles(fa.Obstacles([fa.HalfSpace((0, 0, 0), (0, 0, 1), 1e3, friction=0.5)], slip_velocity=0.1))
    assert con.energy() > 0.0                                                        # (the engine's obstacles stayed)


@pytest.mark.gpu
def test_slip_velocity_and_first_order_refusals(engine):
    asm = _assembler(engine, "HEX8_3", "elastic")
    lib = engine._lib
    code = lambda rc: _code(engine._check, rc)
    rough = fa.Obstacles([fa.HalfSpace((0, 0, 0.1), (0, 0, 1), 1e3, friction=0.5)], slip_length=1e-3, slip_velocity=0.1)
    smooth = fa.Obstacles([fa.HalfSpace((0, 0, 0.1), (0, 0, 1), 1e3)])
    ti = fa.CentralDifference(asm, RHO, 1e-3).with_obstacles(rough)
    for bad in (0.0, -0.1, np.nan, np.inf):
        assert code(lib.fh_dynamics_set_slip_velocity(ti._handle(), bad)) == FH_BAD_ARGUMENT
    assert code(lib.fh_dynamics_set_slip_velocity(ti._handle(), 0.2)) == 0
    ti.close()
    n = 3 * engine.num_nodes()
    for make in (lambda: fa.ForwardEuler(asm, RHO, 1e-4), lambda: fa.RungeKuttaLegendre(asm, RHO, 1e-3, 3), lambda: fa.ThetaMethod(asm, RHO, 1e-2, 1.0)):
        fo = make().with_obstacles(rough)
        assert code(lib.fh_dynamics_set_slip_velocity(fo._handle(), 0.2)) == FH_BAD_ARGUMENT      # a first-order handle
        fo.set_state(np.zeros(n))
        assert _code(fo.step, 1) == FH_UNSUPPORTED
        fo.with_obstacles(smooth)                                                                  # every mu = 0: as before
        assert _code(fo.step, 1) == 0
        fo.close()


@pytest.mark.gpu
def test_eigs_stable_dt_and_the_operator_leave_the_term_out(engine):
    """fh_dynamics_stable_dt and fh_eigs_lowest give the bits of the frictionless run; the operator's own map too"""
    kind = "HEX8_3"
    obs, mu, ubar, u, w, node = _scene(kind)
    small = 0.05 * u
    asm = _assembler(engine, kind, "elastic", small)
    n = small.size
    x = np.random.default_rng(3).uniform(-1.0, 1.0, n)

    def run(friction):
        o = _fa_obstacles(obs, mu if friction else None, w, slip_length=EPS, slip_velocity=0.1)
        ti = fa.CentralDifference(asm, RHO, 1e-3).with_obstacles(o)
        ti.set_state(small)
        out = [np.array(ti.stable_dt(12))]
        ti.close()
        es = fa.MatrixFreeEigensolver(asm, RHO).with_obstacles(o)
        out.append(np.asarray(es.solve(2).values))
        engine.set_obstacles(o)
        out.append(fa.MatrixFreeOperator(asm).apply(np.zeros(n), x).copy())
        return out

    for p, q in zip(run(False), run(True)):
        assert np.array_equal(p, q)


@pytest.mark.gpu
def test_no_launch_is_added_on_the_tiles(engine):
    """fh_last_kernel_name of a central-difference launch and of the tangent's map on the tiles: the names of the frictionless run"""
    u0, v0, f, _ = _slide_state()
    names = {}
    for friction in (False, True):
        obstacles = _fa_obstacles(SLIDE_FLOOR, [SLIDE_MU] if friction else None, slip_velocity=SLIDE_EPS_V, slip_length=1e-3)
        asm = _assembler(engine, BLOCK, "elastic", u0)
        ti = fa.CentralDifference(asm, RHO, SLIDE_DT).with_load(f).with_obstacles(obstacles)
        ti.set_state(u0, v0)
        ti.state()        # a_0: the step's launch, read before a record's energy pass replaces the name
        step_name = engine.last_kernel_name()
        ti.step(4)
        ti.close()
        t = fa.MatrixFreeTangent(asm).with_obstacles(obstacles)
        t.apply(np.zeros_like(u0), v0)
        names[friction] = (step_name, engine.last_kernel_name())
    print(names)
    assert names[True] == names[False] == ("k_element_pass_tiled + k_dynamics_from_partials", "k_element_pass_tiled + k_operator_from_partials")


@pytest.mark.gpu
def test_slide_off_the_tiles(engine, oracle):
    """central differences on a rule-set table (Tet4, two rules): the residual is summed off the tiles and k_contact_force adds g and q with
    the same slip source, dt v_h at the current position: 16 steps against the reference, cut as 16 and 8 + 8"""
    m, w, p = _mesh("TET4")
    w2, p2 = (np.asarray(a) for a in quadrature.total_order.tetrahedron(3))
    emap = (np.arange(m.num_elements()) % 3 == 0).astype(np.uint64)
    conn = np.asarray(m.connectivity)
    floor = [("half_space", (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), SLIDE_K)]

    def problem(dtype=np.float64):
        groups = [(conn[emap == 0], w, p), (conn[emap == 1], w2, p2)]
        if dtype is np.longdouble:
            return fr.LongDoubleElastic("TET4", m.vertices, groups, LAME.mu, LAME.lambda_, RHO, None, floor)
        return cr.ContactProblem(oracle, OKIND["TET4"], oracle.LINEAR_ELASTIC, m.vertices, groups, params=LAME.as_pair(), rho=RHO, obstacles=floor)

    n = m.vertices.size
    u0 = np.zeros(n)
    u0[2::3] = -2e-3
    v0 = np.zeros(n)
    v0[0::3], v0[1::3] = SLIDE_V0, 0.03                 # (0.03: within the smoothing zone eps_v = 0.05 along y alone)
    steps = 16

    def reference(dtype=np.float64):
        return fr.central_difference(fr.FrictionProblem(problem(dtype), [SLIDE_MU], None, None, dtype), u0, v0, SLIDE_DT, steps, SLIDE_EPS_V)[:3]

    ref = reference()
    d_ld = [_rel(np.asarray(a, dtype=np.float64), b) for a, b in zip(reference(dtype=np.longdouble), ref)]
    bound = [_bound(d) for d in d_ld]
    frictionless = dr.central_difference(problem(), u0, v0, SLIDE_DT, steps)[:3]
    assert _rel(frictionless[1], ref[1]) > 1e-3          # the friction term matters in this run
    qt = fa.compact_quadrature_table([p, p2], [w, w2], [[LAME] * len(w), [LAME] * len(w2)], emap)

    def run(chunks):
        asm = _assembler(engine, "TET4", "elastic", qt=qt)
        ti = fa.CentralDifference(asm, RHO, SLIDE_DT).with_obstacles(_fa_obstacles(floor, [SLIDE_MU], slip_velocity=SLIDE_EPS_V))
        ti.set_state(u0, v0)
        ti.state()
        name = engine.last_kernel_name()
        for c in chunks:
            ti.step(c)
        out = ti.state()[:3]
        ti.close()
        return out, name

    got, name = run([steps])
    print(f"off the tiles: d_ld (u, v, a) {d_ld[0]:.2e} {d_ld[1]:.2e} {d_ld[2]:.2e}; kernel {name}")
    assert "k_contact_force" in name and "from_partials" not in name, name
    for what, a, b, bd in zip("uva", got, ref, bound):
        _check(f"slide off the tiles {what}", _rel(a, b), bd)
    again, _ = run([8, 8])
    for a, b in zip(got, again):
        assert np.array_equal(a, b)
