"""Rigid obstacles from sampled signed-distance grids (fh_sdf_grid_*, FH_OBSTACLE_GRID, fenris_amd.SdfGrid / GridObstacle) against the NumPy
statement of tests/sdf_grid_reference.py, which is pinned here on the CPU against central differences of its own energy and force, against
contact_reference's half-space (twin (a): a grid of a linear field) and against a closed form (twin (b): a field of the trilinear space).

Bounds.  The interpolant and the term are short sums per node: 1e-13 max|.| (SHORT_SUM of test_contact.py).  Where the term rides on a
Newton solve or a trajectory the bound is measured from the reference alone as test_contact.py measures its own: d_perm, the reference
under another numbering of the elements, d_newton, the reference under a Newton tolerance 100 times smaller, and the bound
max(20 (d_perm + d_newton), 1e-13).  The constants measured on the CPU are recorded in MEASURED; the tests measure them again and print them.

The device always gets a GRID; the reference of twin (b) is the closed form (a "curved" tuple), so those tests do not depend on any
restatement of the interpolation."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import fenris_amd as fa
from fenris_amd import _ffi

import contact_reference as cr
import dynamics_reference as dr
import motion_reference as mr
import sdf_grid_reference as sg
import test_contact as tc

SHORT_SUM = tc.SHORT_SUM
FH_BAD_ARGUMENT, FH_INVALID_STATE, FH_UNSUPPORTED = 2, 5, 6
NEW = ("fh_sdf_grid_create", "fh_sdf_grid_destroy", "fh_sdf_grid_info", "fh_sdf_grid_sample_dev")
H3 = (0.45, 0.37, 0.31)          # unequal spacings and counts: a transposed index or a swapped axis shows
BOX_ORIGIN, BOX_SHAPE = (-0.25, -0.25, -0.25), (5, 6, 6)    # a box over the unit cube and a margin: up to (1.55, 1.6, 1.3)
EPS = 2.0e-3

# measured on the CPU with the reference alone: (d_perm, d_newton, bound = max(20 (d_perm + d_newton), 1e-13)); the tests measure them again
MEASURED = {"pressed HEX8 elastic, grid floor": (1.7e-16, 1.0e-15, 1.0e-13),
            "warped HEX8 elastic": (1.4e-15, 9.4e-14, 1.9e-12), "warped HEX8 neo_hookean": (9.0e-16, 4.2e-13, 8.4e-12),   # (Gauss-Newton: linear convergence, so the tolerance shows)
            "newmark on the warped floor, 4 steps": (2.6e-15, 3.9e-08, 7.8e-07), "euler on the warped floor, 4 steps": (2.2e-14, 1.2e-08, 2.4e-07),   # (... and in a_n over dt^2)
            "drop on the warped floor, 64 steps": (1.1e-14, 0.0, 2.3e-13), "moving frictional warped floor, 64 steps": (1.2e-14, 0.0, 2.5e-13)}

engine = tc.engine


# ------------------------------------------------------------------------------------------ scenes
def _random_grid(d):
    rng = np.random.default_rng(41)
    if d == 3:
        return ("grid", (0.4, -0.2, -0.4), (rng.uniform(-0.35, 0.35, (4, 5, 6)), H3), 3.0e3)      # x < 0.4 is outside its box
    return ("grid", (0.2, -0.05), (rng.uniform(-0.35, 0.35, (5, 4)), H3[:2]), 3.0e3)               # x < 0.2 is outside


def _curved(d, k=4.0e3):
    return ("curved", (0.5, 0.5, 0.35), 0.4, k) if d == 3 else ("curved", (0.5, 0.4), 0.4, k)


def _mixed(d):
    """a random grid whose box covers part of the mesh, twin (b), a ball and a half-space"""
    return [_random_grid(d), _curved(d), ("ball", (1.1,) * d, 0.7, 2.0e3), ("half_space", (0.3,) * d, (1.0, 2.0, 3.0)[:d], 1.0e4)]


@functools.lru_cache(maxsize=None)
def _curved_values(x0, c, d):
    return sg.sample(sg.curved_field(x0, c), BOX_ORIGIN[:d], H3[:d], BOX_SHAPE[:d])


@functools.lru_cache(maxsize=None)
def _linear_values(p0, nu, d):
    return sg.sample(sg.linear_field(p0, np.asarray(nu) / np.linalg.norm(nu)), BOX_ORIGIN[:d], H3[:d], BOX_SHAPE[:d])


_UPLOADS = {}


def _sdf(values, spacing):
    """one fa.SdfGrid per array of samples"""
    if id(values) not in _UPLOADS:
        _UPLOADS[id(values)] = (values, fa.SdfGrid(values, spacing))
    return _UPLOADS[id(values)][1]


def _fa_obstacles(obstacles, mu=None, paths=None, node_weights=None, linear_as_grid=False, **kw):
    """the device's obstacles: a "curved" tuple becomes the GRID of its field over the box (the path moves box and field alike); with
    linear_as_grid a "half_space" becomes the grid of its linear field"""
    out = []
    for j, (kind, p, q, k) in enumerate(obstacles):
        d = len(p)
        fr_ = 0.0 if mu is None else mu[j]
        path = None if paths is None or paths[j] is None else fa.ObstaclePath(*paths[j])
        if kind == "grid":
            out.append(fa.GridObstacle(_sdf(*q), p, k, friction=fr_, path=path))
        elif kind == "curved":
            out.append(fa.GridObstacle(_sdf(_curved_values(tuple(p), q, d), H3[:d]), BOX_ORIGIN[:d], k, friction=fr_, path=path))
        elif kind == "half_space" and linear_as_grid:
            out.append(fa.GridObstacle(_sdf(_linear_values(tuple(p), tuple(q), d), H3[:d]), BOX_ORIGIN[:d], k, friction=fr_, path=path))
        else:
            cls = fa.HalfSpace if kind == "half_space" else fa.Ball if kind == "ball" else fa.Cavity
            out.append(cls(p, q, k, friction=fr_, path=path))
    return fa.Obstacles(out, node_weights, **kw)


def _assert_inputs(obstacles, X, u, coverage=True):
    """every (node, obstacle) pair is 1e-6 clear of phi = 0 and, in cell units, of every cell face; every obstacle has 3 active nodes and 3
    inactive ones inside its box, the first grid (coverage) 3 nodes outside"""
    phi = sg.phi_table(obstacles, X, u)
    finite = np.isfinite(phi)
    assert np.abs(phi[finite]).min() >= 1e-6, np.abs(phi[finite]).min()
    for row, fin in zip(phi, finite):
        assert (row[fin] < 0).sum() >= 3 and (row[fin] > 0).sum() >= 3, ((row[fin] < 0).sum(), (row[fin] > 0).sum())
    clear = sg.cell_clearance(obstacles, X, u)
    for inside, c in clear:
        assert c >= 1e-6, c
    if coverage and clear:
        assert (~clear[0][0]).sum() >= 3 and clear[0][0].sum() >= 6, clear[0][0].sum()


def _problem(oracle, kind, op, obstacles=(), dirichlet=(), f=None, perm=None, node_weights=None):
    m, w, p = tc._mesh(kind)
    groups = [(np.asarray(m.connectivity), w, p)]
    if perm is not None:
        groups = [(c[np.random.default_rng(perm + g).permutation(len(c))], wg, pg) for g, (c, wg, pg) in enumerate(groups)]
    return sg.GridContactProblem(oracle, tc._okind(kind), tc._oop(oracle, op), m.vertices, groups, params=tc.LAME.as_pair(), rho=tc.RHO,
                                 dirichlet=dirichlet, f=f, obstacles=obstacles, node_weights=node_weights)


_rel, _check, _code = tc._rel, tc._check, tc._code


def _measured(key, d_perm, d_newton):
    bound = max(20.0 * (d_perm + d_newton), 1e-13)
    print(f"{key}: d_perm {d_perm:.2e} d_newton {d_newton:.2e} bound {bound:.2e} (recorded {MEASURED.get(key)})")
    return bound


# ------------------------------------------------------------------------------------------ no GPU: declarations
def test_grid_entry_points_are_declared():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "fenris_hip.h")).read()
    for name in NEW:
        assert name in _ffi.exported_symbols() and name + "(" in hdr
    for text in ("FH_OBSTACLE_HALF_SPACE = 0, FH_OBSTACLE_BALL = 1, FH_OBSTACLE_CAVITY = 2, FH_OBSTACLE_GRID = 3", "#define FH_MAX_SDF_GRIDS 16",
                 "    int grid;", "#define FH_ABI_VERSION 1"):
        assert text in hdr, text
    assert fa.contact.OBSTACLE_GRID == 3 and fa.GridObstacle.kind == 3
    assert C.sizeof(_ffi.Obstacle) == 72 and _ffi.Obstacle.stiffness.offset == 8 and _ffi.Obstacle.grid.offset == 4
    import subprocess
    import sys

    assert subprocess.run([sys.executable, os.path.join(root, "scripts", "gen_rust_bindings.py"), "--check"], capture_output=True).returncode == 0
    rs = open(os.path.join(root, "bindings", "fenris_hip_sys.rs")).read()
    assert "pub grid: c_int," in rs and "pub fn fh_sdf_grid_create(" in rs and "FH_OBSTACLE_GRID: c_int = 3" in rs
    for name in ("SdfGrid", "GridObstacle", "sdf_circle", "sdf_box", "sdf_union"):
        assert hasattr(fa, name)
    assert callable(fa.Contact.sample_grid)


def test_python_grid_helpers():
    """the layout of the upload, from_function, and the formulas of sdf.rs"""
    v = np.arange(24.0).reshape(2, 3, 4)
    g = fa.SdfGrid(v, (0.5, 0.25, 0.125))
    flat = g.abi_values()
    for ix, iy, iz in [(1, 2, 3), (0, 1, 2), (1, 0, 0)]:
        assert flat[(iz * 3 + iy) * 2 + ix] == v[ix, iy, iz]
    circle, box = fa.sdf_circle((0.5, 0.5), 0.25), fa.sdf_box((0.0, 0.0), (1.0, 0.5))
    pts = np.array([[0.5, 0.5], [1.0, 0.5], [2.0, 0.25], [0.5, 0.25], [2.0, 1.5]])
    assert np.allclose(circle(pts), [-0.25, 0.25, np.sqrt(1.5 ** 2 + 0.25 ** 2) - 0.25, 0.0, np.sqrt(1.5 ** 2 + 1.0) - 0.25])
    assert np.allclose(box(pts), [0.0, 0.0, 1.0, -0.25, np.sqrt(2.0)])
    assert np.array_equal(fa.sdf_union(circle, box)(pts), np.minimum(circle(pts), box(pts)))
    ball3 = fa.sdf_circle((0.0, 0.0, 0.0), 1.0)
    assert np.allclose(ball3(np.array([[0.0, 0.0, 3.0]])), [2.0]) and np.allclose(fa.sdf_box((0, 0, 0), (2, 2, 2))(np.array([[1.0, 1.0, 1.5]])), [-0.5])
    grid, origin = fa.SdfGrid.from_function(circle, (-0.5, -0.25), (1.5, 1.25), (9, 7))
    assert grid.shape == (9, 7) and np.array_equal(origin, [-0.5, -0.25]) and np.allclose(grid.spacing, [0.25, 0.25])
    assert grid.values[4, 3] == circle(np.array([[0.5, 0.5]]))[0]
    phi, grad = grid.evaluate(np.array([[0.5, 0.5], [-0.5, -0.25], [1.5, 1.25], [1.6, 0.0], [np.nan, 0.0]]), origin)
    assert phi[0] == -0.25 and phi[1] == circle(np.array([[-0.5, -0.25]]))[0] and phi[2] == circle(np.array([[1.5, 1.25]]))[0]
    assert np.isinf(phi[3:]).all() and not grad[3:].any()
    for bad in (lambda: fa.SdfGrid(np.zeros((1, 3)), (1, 1)), lambda: fa.SdfGrid(np.zeros((2, 2)), (1, 0)), lambda: fa.SdfGrid(np.zeros(4), (1,)),
                lambda: fa.SdfGrid(np.full((2, 2), np.nan), (1, 1)), lambda: fa.GridObstacle(grid, (0, 0, 0), 1.0)):
        with pytest.raises((ValueError, TypeError)):
            bad()


# ------------------------------------------------------------------------------------------ no GPU: the reference pinned
@pytest.mark.parametrize("kind", ["HEX8", "QUAD4"])
def test_reference_force_and_tangent_against_central_differences(kind):
    """g against central differences of E_c and the exact tangent (Gauss-Newton plus k w p Hess phi) against central differences of g; the
    applied block is symmetric positive semi-definite and is the exact one minus the curvature terms"""
    m = tc._mesh(kind)[0]
    d = m.vertices.shape[1]
    rg = _random_grid(d)
    obs = [rg, ("grid", BOX_ORIGIN[:d], (_curved_values(_curved(d)[1], 0.4, d), H3[:d]), 4.0e3)] + _mixed(d)[2:]
    u = tc._random_u(m)
    w = np.random.default_rng(8).uniform(0.5, 2.0, len(m.vertices))
    _assert_inputs(obs, m.vertices, u)
    g = sg.force(obs, m.vertices, u, w)
    B = sg.tangent(obs, m.vertices, u, w, exact=True).toarray()
    h = 1e-6
    fd_g, fd_B = np.zeros_like(g), np.zeros_like(B)
    for i in range(len(u)):
        e = np.zeros_like(u)
        e[i] = h
        fd_g[i] = (sg.energy(obs, m.vertices, u + e, w) - sg.energy(obs, m.vertices, u - e, w)) / (2 * h)
        fd_B[:, i] = (sg.force(obs, m.vertices, u + e, w) - sg.force(obs, m.vertices, u - e, w)) / (2 * h)
    _check(f"{kind} g vs dE_c", _rel(fd_g, g), 2e-9)
    _check(f"{kind} B vs dg", _rel(fd_B, B), 2e-9)
    for ob in obs[:2]:
        applied, exact = sg.blocks([ob], m.vertices, u, w), sg.blocks([ob], m.vertices, u, w, exact=True)
        assert np.abs(applied - applied.transpose(0, 2, 1)).max() <= 1e-12 * ob[3]
        assert min(np.linalg.eigvalsh(b).min() for b in applied) >= -1e-12 * ob[3]
        assert min(np.linalg.eigvalsh(b).min() for b in exact) < 0.0                     # (why the curvature is dropped: indefinite)
        assert np.abs(np.einsum("nii->ni", exact - applied)).max() == 0.0                # ... with a zero diagonal


@pytest.mark.parametrize("kind", ["HEX8", "QUAD4"])
def test_twin_a_is_the_half_space_in_the_reference(kind):
    m = tc._mesh(kind)[0]
    d = m.vertices.shape[1]
    hs = ("half_space", (0.3,) * d, (1.0, 2.0, 3.0)[:d], 1.0e4)
    grid = ("grid", BOX_ORIGIN[:d], (_linear_values(hs[1], hs[2], d), H3[:d]), hs[3])
    u = tc._random_u(m)
    w = np.random.default_rng(8).uniform(0.5, 2.0, len(m.vertices))
    _assert_inputs([grid], m.vertices, u, coverage=False)
    assert sg.cell_clearance([grid], m.vertices, u)[0][0].all()
    for name, f in (("phi", lambda o: sg.phi_table(o, m.vertices, u)), ("energy", lambda o: np.array([sg.energy(o, m.vertices, u, w)])),
                    ("force", lambda o: sg.force(o, m.vertices, u, w)), ("blocks", lambda o: sg.blocks(o, m.vertices, u, w)),
                    ("exact blocks", lambda o: sg.blocks(o, m.vertices, u, w, exact=True))):
        _check(f"{kind} twin (a) {name}", _rel(f([grid]), f([hs])), 1e-13)


@pytest.mark.parametrize("kind", ["HEX8", "QUAD4"])
def test_twin_b_is_the_closed_form_in_the_reference(kind):
    m = tc._mesh(kind)[0]
    d = m.vertices.shape[1]
    curved = _curved(d)
    grid = ("grid", BOX_ORIGIN[:d], (_curved_values(curved[1], curved[2], d), H3[:d]), curved[3])
    u = tc._random_u(m)
    _assert_inputs([grid], m.vertices, u, coverage=False)
    gn = [np.linalg.norm(sg.closed_form(curved[1], curved[2], x)[1]) for x in sg.positions(m.vertices, u)]
    assert max(abs(np.array(gn) - 1.0)) > 0.01                                            # |grad phi| != 1
    for name, f in (("phi", lambda o: sg.phi_table(o, m.vertices, u)), ("force", lambda o: sg.force(o, m.vertices, u)),
                    ("blocks", lambda o: sg.blocks(o, m.vertices, u)), ("exact blocks", lambda o: sg.blocks(o, m.vertices, u, exact=True))):
        _check(f"{kind} twin (b) {name}", _rel(f([grid]), f([curved])), 1e-13)


@pytest.mark.parametrize("d", [2, 3])
def test_python_evaluate_agrees_with_the_reference(d):
    rng = np.random.default_rng(5)
    for trial in range(3):
        shape = tuple(rng.integers(2, 6, d))
        values, h, origin = rng.uniform(-1.0, 1.0, shape), rng.uniform(0.2, 0.6, d), rng.uniform(-0.5, 0.5, d)
        extent = h * (np.array(shape) - 1)
        pts = origin + rng.uniform(-0.15, 1.15, (200, d)) * extent
        phi, grad = fa.SdfGrid(values, h).evaluate(pts, origin)
        outside = 0
        for x, p, g in zip(pts, phi, grad):
            inside, pr, mr_, _, _, _ = sg.interpolate(values, h, origin, x)
            if not inside:
                outside += 1
                assert np.isinf(p) and p > 0 and not g.any()
            else:
                assert abs(p - pr) <= 1e-13 and np.abs(g - mr_).max() <= 1e-13 * max(1.0, np.abs(mr_).max())
        assert 20 <= outside <= 180


# ------------------------------------------------------------------------------------------ GPU 1: the interpolant alone
def _t_of(x, o, h):
    return (x - o) / h


def _probe_points(values, h, origin):
    """random points, every sample position, points on the last faces (t == n - 1 exactly) and one ulp outside each face"""
    d, n = values.ndim, np.array(values.shape)
    h, origin = np.asarray(h, dtype=np.float64), np.asarray(origin, dtype=np.float64)
    rng = np.random.default_rng(17)
    extent = h * (n - 1)
    pts = [origin + rng.uniform(-0.1, 1.1, (300, d)) * extent]
    idx = np.stack(np.meshgrid(*[np.arange(k) for k in n], indexing="ij"), axis=-1).reshape(-1, d)
    pts.append(origin + idx * h)
    inner = origin + rng.uniform(0.05, 0.95, (8 * d, d)) * extent
    on_face, outside = [], []
    for a in range(d):
        hi = origin[a] + (n[a] - 1) * h[a]
        while _t_of(hi, origin[a], h[a]) > n[a] - 1:
            hi = np.nextafter(hi, -np.inf)
        while _t_of(np.nextafter(hi, np.inf), origin[a], h[a]) <= n[a] - 1:
            hi = np.nextafter(hi, np.inf)
        # hi: the largest x_a inside.  t == n - 1 exactly wherever a double gives it (every axis here but y of the 5 x 4 grid, where
        # 3 * 0.37 has no such x: there t is one ulp below n - 1, the last point of the last cell)
        t_hi = _t_of(hi, origin[a], h[a])
        assert t_hi == n[a] - 1 or (d == 2 and a == 1 and t_hi == np.nextafter(float(n[a] - 1), 0.0)), (a, t_hi)
        for j, value in enumerate((hi, origin[a], np.nextafter(hi, np.inf), np.nextafter(origin[a], -np.inf))):
            q = inner[4 * a:4 * a + 4].copy()
            q[:, a] = value
            (on_face if j < 2 else outside).append(q)
    return np.concatenate(pts + on_face + outside), sum(len(q) for q in outside)


@pytest.mark.gpu
@pytest.mark.parametrize("d", [2, 3])
def test_sample_grid(engine, d):
    rng = np.random.default_rng(23)
    shape, h, origin = ((4, 5, 6), H3, (0.3, -0.2, 0.7)) if d == 3 else ((5, 4), H3[:2], (0.3, -0.2))
    values = rng.uniform(-1.0, 1.0, shape)
    grid = fa.SdfGrid(values, h)
    pts, n_out = _probe_points(values, h, origin)
    phi_ref, grad_ref = np.full(len(pts), np.inf), np.zeros((len(pts), d))
    for i, x in enumerate(pts):
        inside, p, m, _, _, _ = sg.interpolate(values, h, origin, x)
        if inside:
            phi_ref[i], grad_ref[i] = p, m
    assert np.isinf(phi_ref[-n_out:]).all() and np.isfinite(phi_ref[-2 * n_out:-n_out]).all() and 20 <= np.isinf(phi_ref[:300]).sum() <= 200
    phi, grad = fa.Contact(engine).sample_grid(grid, origin, pts)
    assert engine.last_kernel_name() == "k_sdf_grid_sample"
    assert np.array_equal(np.isinf(phi), np.isinf(phi_ref)) and (phi[np.isinf(phi)] > 0).all() and not grad[np.isinf(phi)].any()
    fin = np.isfinite(phi_ref)
    _check(f"{d}-D phi", np.abs(phi[fin] - phi_ref[fin]).max(), SHORT_SUM)
    _check(f"{d}-D grad", np.abs(grad[fin] - grad_ref[fin]).max() / np.abs(grad_ref).max(), SHORT_SUM)
    ph, gh = grid.evaluate(pts, origin)
    assert np.array_equal(np.isinf(ph), np.isinf(phi_ref)) and np.abs(ph[fin] - phi_ref[fin]).max() <= SHORT_SUM
    # a sample comes back to the bit at its position wherever t is a whole number on every axis (f == 0: the other corners get weight 0)
    nodes = np.arange(300, 300 + values.size)
    whole = np.array([bool(np.all(sg.interpolate(values, h, origin, pts[i])[5] == 0.0)) for i in nodes])
    assert whole.sum() >= 8 and np.array_equal(phi[nodes][whole], values.reshape(-1)[whole])


# ------------------------------------------------------------------------------------------ GPU 2: the term
def _term_scene(kind, obstacles=None):
    """obstacles (default: the mixed four) with paths on three of them, coefficients, node weights, a lag state, a u with slips on both sides
    of EPS and a clock inside two different segments"""
    X = np.asarray(tc._mesh(kind)[0].vertices)
    N, d = X.shape
    rng = np.random.default_rng(31)
    obs = _mixed(d) if obstacles is None else obstacles
    paths = [([0.0, 1.0, 2.0], [[0.0] * d, [0.015625, 0.0078125, 0.03125][:d], [0.03125, -0.0078125, 0.015625][:d]]),
             ([0.5, 1.5], [[0.0] * d, [-0.03125, 0.015625, -0.015625][:d]]), None, ([0.0, 2.0], [[0.0] * d, [0.03125, -0.015625, 0.0078125][:d]])][:len(obs)]
    mu = [0.5, 0.3, 0.7, 0.2][:len(obs)]
    w = rng.uniform(0.5, 2.0, N)
    ubar = rng.uniform(-0.02, 0.02, N * d)
    u = ubar + (rng.uniform(-0.02, 0.02, (N, d)) * rng.choice([0.1, 1.0], (N, 1))).reshape(-1)
    return obs, paths, mu, w, ubar, u, (1.25, 0.75)


def _device_items(engine, kind, op, scene, **kw):
    """every stand-alone piece of the term on the device, by name"""
    import torch

    obs, paths, mu, w, ubar, u, (t, t_lag) = scene
    m = tc._mesh(kind)[0]
    n = m.vertices.size
    asm = tc._assembler(engine, kind, op, u)
    out = {}
    engine.set_obstacles(_fa_obstacles(obs, None, paths, w, **kw))
    engine.set_obstacle_time(t, t_lag)
    con = fa.Contact(engine)
    out["energy"] = np.array([con.energy()])
    out["gap"] = con.gap()
    garbage = np.random.default_rng(5).uniform(-1.0, 1.0, n + 64)
    buf = torch.tensor(garbage, device="cuda:0")
    con.force(device=True, out=buf[32:32 + n])
    got = buf.cpu().numpy()
    assert np.array_equal(got[:32], garbage[:32]) and np.array_equal(got[32 + n:], garbage[32 + n:])
    out["force into garbage"] = got[32:32 + n] - garbage[32:32 + n]
    out["force"] = con.force()
    out["csr blocks"] = tc._csr_of_contact(engine, asm)
    out["resultants"] = con.resultants()[0]
    x = np.random.default_rng(6).uniform(-1.0, 1.0, n)
    tan = fa.MatrixFreeTangent(asm).with_obstacles(_fa_obstacles(obs, None, paths, w, **kw))
    engine.set_obstacle_time(t, t_lag)
    y1 = tan.apply(np.zeros(n), x).copy()
    out["route"] = engine.last_kernel_name()
    d1 = tan.diagonal()
    tan.with_obstacles(None)
    y0, d0 = tan.apply(np.zeros(n), x).copy(), tan.diagonal()
    out["apply difference"], out["diagonal difference"], out["apply scale"], out["diagonal scale"] = y1 - y0, d1 - d0, np.abs(y0).max(), np.abs(d1).max()
    # friction: the lag state, the clock, the obstacle's own displacement over the lag interval
    engine.set_obstacles(_fa_obstacles(obs, mu, paths, w, slip_length=EPS, **kw))
    engine._check(engine._lib.fh_set_friction_reference(engine._h, _ffi.fp(np.ascontiguousarray(ubar))))
    engine.set_obstacle_time(t, t_lag)
    out["friction potential"] = np.array([con.friction_potential()])
    out["friction force"] = con.friction_force()
    out["csr blocks with friction"] = tc._csr_of_contact(engine, asm)
    out["friction resultants"] = con.resultants()[1]
    engine.set_obstacles(None)
    return out, x


def _reference_items(kind, scene, x):
    obs, paths, mu, w, ubar, u, (t, t_lag) = scene
    X = np.asarray(tc._mesh(kind)[0].vertices)
    d = X.shape[1]
    cur, lag, c = mr.placed(obs, paths, t), mr.placed(obs, paths, t_lag), mr.displacements(paths, t, t_lag)
    _assert_inputs(cur, X, u)
    _assert_inputs(lag, X, ubar)
    B = sg.tangent(cur, X, u, w).toarray()
    H = mr.friction_tangent(lag, mu, X, ubar, u - ubar, c, EPS, w).toarray()
    R, Q = mr.resultants(cur, X, u, w, mu, lag, ubar, u - ubar, c, EPS)
    g = sg.force(cur, X, u, w)
    return {"energy": np.array([sg.energy(cur, X, u, w)]), "gap": sg.gap(cur, X, u), "force into garbage": g, "force": g, "csr blocks": B,
            "resultants": R, "apply difference": B @ x, "diagonal difference": B.diagonal(),
            "friction potential": np.array([mr.friction_potential(lag, mu, X, ubar, u - ubar, c, EPS, w)]),
            "friction force": mr.friction_force(lag, mu, X, ubar, u - ubar, c, EPS, w), "csr blocks with friction": B + H, "friction resultants": Q}


def _compare_items(tag, got, ref):
    for name, want in ref.items():
        have = got[name]
        assert np.array_equal(np.isinf(have), np.isinf(want)), name
        fin = np.isfinite(want)
        scale = max(np.abs(want[fin]).max(), 1e-300)
        if name == "apply difference":
            scale = max(scale, got["apply scale"])
        if name == "diagonal difference":
            scale = max(scale, got["diagonal scale"])
        if name == "force into garbage":
            scale = max(scale, 1.0)
        _check(f"{tag} {name}", np.abs(have[fin] - want[fin]).max() / scale, SHORT_SUM + (2.3e-16 if name == "force into garbage" else 0.0))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", tc.PARITY_KINDS)
def test_term_parity_with_grids(engine, kind):
    """energy, gap, force, CSR blocks, the tangent's map and diagonal, resultants and the friction potential, force and blocks with a lag
    state and moving obstacles, for a random grid that covers part of the mesh, twin (b), a ball and a half-space together, with weights"""
    scene = _term_scene(kind)
    got, x = _device_items(engine, kind, "neo_hookean", scene)
    ref = _reference_items(kind, scene, x)
    assert np.isinf(ref["gap"]).sum() == 0 and np.abs(ref["friction force"]).max() > 0.0
    one = ([scene[0][0]],) + tuple(s[:1] if isinstance(s, list) else s for s in scene[1:])     # the random grid alone: +inf in the gap outside its box
    X = np.asarray(tc._mesh(kind)[0].vertices)
    assert np.isinf(sg.gap(mr.placed(one[0], one[1], 1.25), X, scene[5])).sum() >= 3
    _compare_items(kind, got, ref)
    if kind == "TET10":
        assert got["route"].endswith("+ k_contact_apply"), got["route"]
    else:
        assert got["route"].endswith("k_operator_from_partials"), got["route"]
    got1, x1 = _device_items(engine, kind, "neo_hookean", one)
    ref1 = sg.gap(mr.placed(one[0], one[1], 1.25), X, scene[5])
    assert np.array_equal(np.isinf(got1["gap"]), np.isinf(ref1)) and (got1["gap"][np.isinf(ref1)] > 0).all()
    outside = np.isinf(ref1)
    d = X.shape[1]
    outside_lag = np.isinf(sg.gap(mr.placed(one[0], one[1], 0.75), X, scene[4]))               # (friction looks at the lag configuration)
    assert outside_lag.sum() >= 3
    assert not got1["force"].reshape(-1, d)[outside].any() and not got1["friction force"].reshape(-1, d)[outside_lag].any()
    assert not got1["diagonal difference"].reshape(-1, d)[outside].any()


# ------------------------------------------------------------------------------------------ GPU 3: twin (a) is the half-space on the device
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["HEX8", "TET10"])
def test_twin_a_is_the_half_space_on_the_device(engine, kind):
    d = 3
    obs = [("half_space", (0.3,) * d, (1.0, 2.0, 3.0), 1.0e4), ("half_space", (0.0, 0.0, 0.25), (0.0, 0.0, 1.0), 5.0e3)]
    scene = _term_scene(kind, obs)
    X = np.asarray(tc._mesh(kind)[0].vertices)
    _assert_inputs(mr.placed(obs, scene[1], 1.25), X, scene[5], coverage=False)
    plain, x = _device_items(engine, kind, "neo_hookean", scene)
    grid, _ = _device_items(engine, kind, "neo_hookean", scene, linear_as_grid=True)
    assert grid["route"] == plain["route"]
    _compare_items(f"{kind} grid vs half-space", grid, {k: v for k, v in plain.items() if k not in ("route", "apply scale", "diagonal scale")})
    assert np.abs(plain["friction force"]).max() > 0.0 and np.abs(plain["force"]).max() > 0.0


def _newton(oracle, engine, kind, op, ref_obs, dev_obstacles, bc, f, u0, tol, key):
    def solve(perm, t):
        prob = _problem(oracle, kind, op, ref_obs, bc, f, perm)

        def F(x):
            out = prob.residual(x) - prob.f
            out[~prob.free] = 0.0
            return out

        st, u, it = dr.newton(prob, F, prob.tangent, u0.copy(), t)
        assert st == "ok", st
        return u, it

    u_ref, it = solve(None, tol)
    bound = _measured(key, _rel(solve(7, tol)[0], u_ref), _rel(solve(None, tol / 100.0)[0], u_ref))
    asm = tc._assembler(engine, kind, op)
    solver = fa.MatrixFreeNewton(asm).with_dirichlet_nodes(bc).with_load(f).with_obstacles(dev_obstacles)
    u = u0.copy()
    res = solver.solve(u, fa.NewtonSettings(60, tol), line_search=fa.BacktrackingLineSearch(), preconditioner=_ffi.PRECOND_JACOBI, linear_rel_tol=1e-13)
    print(f"{key}: reference {it} iterations, device {res.iterations}; |F| {res.residual_norm:.2e}")
    assert res.residual_norm <= tol
    return u, u_ref, bound


@pytest.mark.gpu
def test_newton_pressed_block_on_a_grid_floor(engine, oracle):
    """test_contact.py's pressed block with the floor given as a grid of its linear field"""
    kind, op = "HEX8", "elastic"
    m = tc._mesh(kind)[0]
    n = m.vertices.size
    obs = [("half_space", (0.0, 0.0, 0.02), (0.0, 0.0, 1.0), 1.0e4)]
    top = tc._face(m, 2, 1.0)
    u0 = np.zeros(n)
    u0[3 * top + 2] = -0.05
    u, u_ref, bound = _newton(oracle, engine, kind, op, obs, _fa_obstacles(obs, linear_as_grid=True), top, np.zeros(n), u0, tc.NEWTON_TOLERANCE,
                              "pressed HEX8 elastic, grid floor")
    assert (cr.gap(obs, m.vertices, u_ref) < 0).sum() >= 4
    _check("u", _rel(u, u_ref), bound)


# ------------------------------------------------------------------------------------------ GPU 4: twin (b) through the solvers
WARPED_FLOOR = [("curved", (0.5, 0.5, 0.02), 0.1, 1.0e4)]         # z >= 0.02 + 0.1 (x - 0.5)(y - 0.5)
WARPED_DROP = [("curved", (0.5, 0.5, -0.02), 0.1, 2.0e3)]


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["elastic", "neo_hookean"])
def test_newton_on_a_warped_floor(engine, oracle, op):
    """the cube's top face held at u_z = -0.05 over twin (b): Newton with backtracking; Gauss-Newton, so the convergence is linear"""
    kind = "HEX8"
    m = tc._mesh(kind)[0]
    n = m.vertices.size
    top = tc._face(m, 2, 1.0)
    u0 = np.zeros(n)
    u0[3 * top + 2] = -0.05
    tol = 1e-10
    u, u_ref, bound = _newton(oracle, engine, kind, op, WARPED_FLOOR, _fa_obstacles(WARPED_FLOOR), top, np.zeros(n), u0, tol, f"warped HEX8 {op}")
    assert (sg.gap(WARPED_FLOOR, m.vertices, u_ref) < 0).sum() >= 4
    _check("u", _rel(u, u_ref), bound)


def _drop_dt():
    return tc._drop_dt("HEX8", "neo_hookean")[0]


@pytest.mark.gpu
@pytest.mark.parametrize("scheme", ["newmark", "euler"])
def test_implicit_drop_on_a_warped_floor(engine, oracle, scheme):
    kind, op = "HEX8", "neo_hookean"
    m = tc._mesh(kind)[0]
    dt = 8.0 * _drop_dt()
    u0, v0 = tc._drop_state(m)
    tol = 1e-10

    def reference(perm, t):
        st, u, v, a, rec, done, _ = dr.implicit(_problem(oracle, kind, op, WARPED_DROP, perm=perm), scheme, u0, v0, dt, 4, 2, tol=t)
        assert st == "ok" and done == 4
        return u, v, a, rec

    ref = reference(None, tol)
    bound = _measured(f"{scheme} on the warped floor, 4 steps", tc._traj_rel(reference(7, tol), ref), tc._traj_rel(reference(None, tol / 100.0), ref))
    assert sg.gap(WARPED_DROP, m.vertices, ref[0]).min() < 0.0
    asm = tc._assembler(engine, kind, op)
    ti = (fa.Newmark if scheme == "newmark" else fa.BackwardEuler)(asm, tc.RHO, dt)
    ti.with_newton(fa.NewtonSettings(60, tol), linear_rel_tol=1e-13).with_obstacles(_fa_obstacles(WARPED_DROP))
    ti.set_state(u0, v0)
    rec = ti.step(4, 2)
    u, v, a, _, _ = ti.state()
    ti.close()
    _check(scheme, tc._traj_rel((u, v, a, tc._records(rec)), ref), bound)


@pytest.mark.gpu
def test_central_difference_drop_on_a_warped_floor(engine, oracle):
    """64 steps of the dropped cube onto twin (b), records every 8, against dr.central_difference"""
    kind, op = "HEX8", "neo_hookean"
    m = tc._mesh(kind)[0]
    dt = _drop_dt()
    u0, v0 = tc._drop_state(m)
    ref = dr.central_difference(_problem(oracle, kind, op, WARPED_DROP), u0, v0, dt, 64, 8)
    perm = dr.central_difference(_problem(oracle, kind, op, WARPED_DROP, perm=7), u0, v0, dt, 64, 8)
    bound = _measured("drop on the warped floor, 64 steps", tc._traj_rel(perm, ref), 0.0)
    early = dr.central_difference(_problem(oracle, kind, op, WARPED_DROP), u0, v0, dt, 12, 0)
    assert sg.gap(WARPED_DROP, m.vertices, early[0]).min() < -0.005 and ref[1][2::3].mean() > 0.5       # in the floor at step 12, on the way up at 64
    asm = tc._assembler(engine, kind, op)
    ti = fa.CentralDifference(asm, tc.RHO, dt).with_obstacles(_fa_obstacles(WARPED_DROP))
    ti.set_state(u0, v0)
    rec = ti.step(64, 8)
    u, v, a, _, _ = ti.state()
    name = engine.last_kernel_name()
    ti.close()
    print("kernel", name)
    _check("trajectory", tc._traj_rel((u, v, a, tc._records(rec)), ref), bound)


MOVING_PATH = [([0.0, 1.0], [[0.0, 0.0, 0.0], [0.5, 0.25, 0.5]])]      # the floor slides and rises while the cube falls onto it
EPS_V = 0.05


@pytest.mark.gpu
def test_central_difference_with_friction_on_a_moving_grid(engine, oracle):
    """the same drop with mu = 0.4 on the grid, which moves along a two-knot path: against motion_reference, and 1 + 63 steps give the bytes of
    64 steps"""
    kind, op = "HEX8", "neo_hookean"
    m = tc._mesh(kind)[0]
    dt = _drop_dt()
    u0, v0 = tc._drop_state(m)
    mu = [0.4]

    def reference(perm, mu=mu):
        mp = mr.MovingProblem(_problem(oracle, kind, op, WARPED_DROP, perm=perm), MOVING_PATH, mu)
        return mr.central_difference(mp, u0, v0, dt, 64, 8, eps_v=EPS_V)

    ref = reference(None)
    bound = _measured("moving frictional warped floor, 64 steps", tc._traj_rel(reference(7), ref), 0.0)
    still = dr.central_difference(_problem(oracle, kind, op, WARPED_DROP), u0, v0, dt, 64, 8)
    assert _rel(still[0], ref[0]) > 1e-3 and _rel(reference(None, None)[0], ref[0]) > 1e-3  # the path shows, and so does the friction

    def run(chunks):
        asm = tc._assembler(engine, kind, op)
        ti = fa.CentralDifference(asm, tc.RHO, dt).with_obstacles(_fa_obstacles(WARPED_DROP, mu, MOVING_PATH, slip_velocity=EPS_V))
        ti.set_state(u0, v0)
        rows = [tc._records(ti.step(c, 8)) for c in chunks]
        u, v, a, _, step = ti.state()
        ti.close()
        assert step == 64
        return u, v, a, rows[-1]

    got = run([64])
    _check("trajectory", tc._traj_rel(got, ref), bound)
    cut = run([1, 63])
    for p, q in zip(got[:3], cut[:3]):
        assert np.array_equal(p, q)
    assert np.array_equal(got[3][-1], cut[3][-1])


# ------------------------------------------------------------------------------------------ GPU 5: lifetime and errors
def _create(engine, dim, n, h, values):
    slot = C.c_uint32(99)
    n3, h3 = np.asarray(n, dtype=np.uint32), np.asarray(h, dtype=np.float64)
    rc = engine._lib.fh_sdf_grid_create(engine._h, dim, n3.ctypes.data_as(_ffi.u32p), _ffi.fp(h3), None if values is None else _ffi.fp(values), C.byref(slot))
    return rc, int(slot.value)


@pytest.mark.gpu
def test_grid_lifetime_and_errors(engine):
    lib, h = engine._lib, engine._h
    good = np.linspace(-1.0, 1.0, 24)
    for dim, n, sp, vals in [(1, (4, 1, 1), (1, 1, 1), good), (4, (2, 2, 2), (1, 1, 1), good), (3, (1, 4, 6), (1, 1, 1), good), (2, (4, 1, 1), (1, 1, 1), good),
                             (2, (4, 3, 2), (1, 1, 1), good), (3, (2, 3, 4), (1, 0.0, 1), good), (3, (2, 3, 4), (1, -1.0, 1), good),
                             (3, (2, 3, 4), (1, np.inf, 1), good), (3, (2, 3, 4), (np.nan, 1, 1), good), (3, (2, 3, 4), (1, 1, 1), None),
                             (3, (2, 3, 4), (1, 1, 1), np.where(np.arange(24) == 23, np.nan, good)), (3, (2, 3, 4), (1, 1, 1), np.where(np.arange(24) == 5, np.inf, good)),
                             (3, (2048, 2048, 512), (1, 1, 1), good)]:
        assert _create(engine, dim, n, sp, vals)[0] == FH_BAD_ARGUMENT, (dim, n, sp)
    assert lib.fh_sdf_grid_create(h, 3, None, None, None, None) == FH_BAD_ARGUMENT
    assert _create(engine, 2, (4, 6, 1), (1, 1, np.nan), good) == (0, 0)        # 2-D: spacing[2] is not read
    ids = [_create(engine, 3, (2, 3, 4), (0.5, 0.25, 0.125), good) for _ in range(15)]
    assert ids == [(0, i) for i in range(1, 16)]
    assert _create(engine, 3, (2, 3, 4), (1, 1, 1), good)[0] == FH_UNSUPPORTED  # all 16 slots are taken
    assert lib.fh_sdf_grid_destroy(h, 5) == 0 and lib.fh_sdf_grid_destroy(h, 5) == FH_BAD_ARGUMENT and lib.fh_sdf_grid_destroy(h, 16) == FH_BAD_ARGUMENT
    assert _create(engine, 3, (4, 3, 2), (1.0, 2.0, 3.0), good) == (0, 5)       # a destroyed slot is reused
    dim, n, sp = C.c_uint32(0), np.zeros(3, dtype=np.uint32), np.zeros(3)
    assert lib.fh_sdf_grid_info(h, 5, C.byref(dim), n.ctypes.data_as(_ffi.u32p), _ffi.fp(sp)) == 0
    assert (dim.value, n.tolist(), sp.tolist()) == (3, [4, 3, 2], [1.0, 2.0, 3.0])
    assert lib.fh_sdf_grid_info(h, 17, None, None, None) == FH_BAD_ARGUMENT and lib.fh_sdf_grid_info(h, 5, None, None, None) == 0
    assert lib.fh_sdf_grid_sample_dev(h, 17, _ffi.fp(sp), None, 0, None, None) == FH_BAD_ARGUMENT
    assert lib.fh_sdf_grid_sample_dev(h, 5, _ffi.fp(sp), None, 4, None, None) == FH_BAD_ARGUMENT
    for i in range(16):
        assert lib.fh_sdf_grid_destroy(h, i) == 0

    def obstacle(grid, kind=3):
        o = (_ffi.Obstacle * 1)()
        o[0].kind, o[0].grid, o[0].stiffness = kind, grid, 1.0e3
        return o

    # obstacles that name grids
    assert _create(engine, 3, (2, 3, 4), (0.75, 0.75, 0.75), good) == (0, 0) and _create(engine, 2, (4, 6, 1), (0.5, 0.5, 1), good) == (0, 1)
    assert lib.fh_set_obstacles(h, obstacle(0), 1, None) == FH_INVALID_STATE    # no mesh
    asm = tc._assembler(engine, "HEX8", "elastic", np.full(81, -0.1))
    assert lib.fh_sdf_grid_info(h, 0, None, None, None) == 0                    # a grid survives fh_set_mesh
    floor = fa.HalfSpace((0, 0, 0), (0, 0, 1), 1e3)
    engine.set_obstacles([floor])
    e_floor = fa.Contact(engine).energy()
    assert e_floor > 0.0
    for bad in (obstacle(2), obstacle(-1), obstacle(16), obstacle(1)):           # not live, out of range, a 2-D grid on a 3-D mesh
        assert lib.fh_set_obstacles(h, bad, 1, None) == FH_BAD_ARGUMENT
    assert lib.fh_set_obstacles(h, obstacle(0, kind=7), 1, None) == FH_BAD_ARGUMENT
    assert fa.Contact(engine).energy() == e_floor                               # a failed call leaves the standing list intact
    assert lib.fh_set_obstacles(h, obstacle(2, kind=1), 1, None) == FH_BAD_ARGUMENT   # (a ball of radius 0; its grid field is not read)
    ball = obstacle(12345, kind=1)
    ball[0].radius = 0.5
    assert lib.fh_set_obstacles(h, ball, 1, None) == 0                          # the field is read for FH_OBSTACLE_GRID only
    assert lib.fh_set_obstacles(h, obstacle(0), 1, None) == 0
    e_grid = fa.Contact(engine).energy()
    assert lib.fh_sdf_grid_destroy(h, 0) == FH_INVALID_STATE                    # a standing obstacle refers to it
    assert lib.fh_sdf_grid_destroy(h, 1) == 0                                   # ... but not to this one
    assert lib.fh_set_obstacles(h, obstacle(0), 1, None) == 0 and fa.Contact(engine).energy() == e_grid      # a second fh_set_obstacles
    asm2 = tc._assembler(engine, "HEX8", "elastic", np.full(81, -0.1))          # fh_set_mesh clears the obstacles, not the grids
    assert fa.Contact(engine).energy() == 0.0 and lib.fh_sdf_grid_info(h, 0, None, None, None) == 0
    assert lib.fh_set_obstacles(h, obstacle(0), 1, None) == 0 and fa.Contact(engine).energy() == e_grid
    engine.set_obstacles(None)
    assert lib.fh_sdf_grid_destroy(h, 0) == 0 and lib.fh_set_obstacles(h, obstacle(0), 1, None) == FH_BAD_ARGUMENT
    assert asm is not None and asm2 is not None


@pytest.mark.gpu
def test_two_engines_hold_their_own_uploads(engine):
    d = 3
    curved = _curved(d)
    grid = fa.SdfGrid(_curved_values(curved[1], curved[2], d), H3)
    ob = fa.GridObstacle(grid, BOX_ORIGIN, curved[3])
    m = tc._mesh("HEX8")[0]
    u = tc._random_u(m)
    e_ref = sg.energy([curved], m.vertices, u)
    other = fa.Engine(0)
    try:
        # the other engine's slot 0 is taken by another grid first: the ids of one SdfGrid differ between the engines
        filler = fa.SdfGrid(np.ones((2, 2, 2)), (1.0, 1.0, 1.0))
        fa.Contact(other).sample_grid(filler, (0, 0, 0), np.zeros((1, 3)))
        a1, a2 = tc._assembler(engine, "HEX8", "elastic", u), tc._assembler(other, "HEX8", "elastic", u)
        engine.set_obstacles([ob])
        other.set_obstacles([ob])
        assert grid._id_on(engine) == 0 and grid._id_on(other) == 1
        assert abs(fa.Contact(engine).energy() - e_ref) <= SHORT_SUM * e_ref and fa.Contact(other).energy() == fa.Contact(engine).energy()
        engine.set_obstacles([ob, ob])                                           # one upload per (engine, grid)
        assert grid._id_on(engine) == 0 and engine._lib.fh_sdf_grid_info(engine._h, 1, None, None, None) == FH_BAD_ARGUMENT
        assert a1 is not None and a2 is not None
    finally:
        other.close()
    assert other._sdf_grids == {} and fa.Contact(engine).energy() > e_ref
