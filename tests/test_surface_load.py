"""Surface load vector (fh_assemble_surface_load, fh_physical_face_quadrature_points, SurfaceLoad) against the long-double restatement
of tests/boundary_reference.py (face basis x explicit tangent cross product; the kernel uses the cell's basis and Nanson's formula),
to 1e-12 * max|f| -- the project's vector tolerance.  Then identities that fail when orientation, face basis or measure is wrong:
the divergence-theorem patch test against the residual assembler, closed surfaces, and a Newton solve loaded by a pressure."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import boundary_reference as br  # noqa: E402
import fenris_amd as fa  # noqa: E402
from fenris_amd import _ffi, quadrature  # noqa: E402

P = fa.procedural
KINDS = ["hex", "tet", "quad", "tri", "hex27", "tet10", "quad9", "tri6", "hex20"]
TOL = 1e-12


def _linear(name, n):
    return {"hex": P.create_unit_box_uniform_hex_mesh_3d, "tet": P.create_unit_box_uniform_tet_mesh_3d,
            "quad": P.create_unit_square_uniform_quad_mesh_2d, "tri": P.create_unit_square_uniform_tri_mesh_2d}[name](n)


_BASE = {"hex27": "hex", "hex20": "hex", "tet10": "tet", "quad9": "quad", "tri6": "tri"}
_RAISE = {"hex27": fa.hex27_mesh_from_hex8, "hex20": fa.hex20_mesh_from_hex8, "tet10": fa.tet10_mesh_from_tet4,
          "quad9": fa.quad9_mesh_from_quad4, "tri6": fa.tri6_mesh_from_tri3}


def _distorted(name, n=2, seed=0, move_mid_nodes=True):
    """every corner vertex moved (non-planar Hex8 faces); the quadratic kinds built on the moved corners, then their mid nodes moved
    off the corner geometry -- which must change nothing: the geometry is the corner map"""
    rng = np.random.default_rng(100 + seed)
    lin = _linear(_BASE.get(name, name), n)
    lin = fa.Mesh(lin.vertices + (0.08 / n) * rng.uniform(-1, 1, lin.vertices.shape), lin.connectivity, lin.elem_kind)
    if name not in _BASE:
        return lin
    m = _RAISE[name](lin)
    if move_mid_nodes:
        corners = np.unique(m.connectivity[:, :br.CELL_CORNERS[m.elem_kind]])
        mid = np.setdiff1d(np.arange(m.num_nodes()), corners.astype(np.int64))
        v = m.vertices.copy()
        v[mid] += (0.1 / n) * rng.uniform(-1, 1, (len(mid), v.shape[1]))
        m = fa.Mesh(v, m.connectivity, m.elem_kind)
    return m


def _face_subset(m, seed):
    """a shuffled subset of ALL (cell, local face) pairs: interior faces too, any order"""
    rng = np.random.default_rng(200 + seed)
    nfaces = len(br.FACES[m.elem_kind])
    pairs = np.array([(c, f) for c in range(m.num_elements()) for f in range(nfaces)])
    pick = rng.permutation(len(pairs))[: max(3, (2 * len(pairs)) // 3)]
    return pairs[pick, 0].astype(np.uint64), pairs[pick, 1].astype(np.uint32)


def _cases(m, cells, nq, seed):
    """(label, kind, sdim, data) over traction s = d, traction s = 1 and pressure, each in the three data shapes"""
    rng = np.random.default_rng(300 + seed)
    d, F = m.vertices.shape[1], len(cells)
    out = []
    for label, kind, s, comps in (("traction", _ffi.LOAD_TRACTION, d, d), ("traction-scalar", _ffi.LOAD_TRACTION, 1, 1),
                                  ("pressure", _ffi.LOAD_PRESSURE, d, 1)):
        for count in (1, F, F * nq):
            out.append((f"{label}/{count}", kind, s, rng.uniform(-2, 2, count * comps), count))
    return out


def _reference(m, cells, lfs, w, p, kind, s, data):
    kw = {"pressure": data} if kind == _ffi.LOAD_PRESSURE else {"traction": data}
    return br.surface_load(m.elem_kind, m.vertices, m.connectivity, cells, lfs, w, p, s, **kw)


# ------------------------------------------------------------------------------------------------------------------- no GPU
@pytest.mark.parametrize("name", KINDS)
def test_checker_agrees_with_a_higher_order_rule(name):
    """the inputs of the GPU comparison below, on the CPU: the checker with the rule used there and with a richer one agree to the
    tolerance (tractions on warped quadrilaterals integrate |a|, which is not a polynomial: the rule must resolve it)"""
    m = _distorted(name)
    cells, lfs = _face_subset(m, 0)
    fk = br.FACE_KIND[m.elem_kind]
    (w, p), (w2, p2) = br.face_rule(fk, _rule_points(name)), br.face_rule(fk, _rule_points(name) + 3)
    d = m.vertices.shape[1]
    rng = np.random.default_rng(7)
    for kind, s, data in ((_ffi.LOAD_TRACTION, d, rng.uniform(-2, 2, d)), (_ffi.LOAD_PRESSURE, d, rng.uniform(-2, 2, len(cells)))):
        a, b = _reference(m, cells, lfs, w, p, kind, s, data), _reference(m, cells, lfs, w2, p2, kind, s, data)
        err = float(np.abs(a - b).max() / np.abs(b).max())
        print(f"{name} kind={kind}: rule {_rule_points(name)} vs {_rule_points(name) + 3}: rel.err {err:.2e}")
        assert err <= TOL


def _rule_points(name):
    return 7 if name in ("hex", "hex27", "hex20") else 4


def test_moved_mid_nodes_change_nothing_in_the_checker():
    for name in _BASE:
        a, b = _distorted(name, move_mid_nodes=True), _distorted(name, move_mid_nodes=False)
        cells, lfs = _face_subset(a, 1)
        w, p = br.face_rule(br.FACE_KIND[a.elem_kind], 3)
        d = a.vertices.shape[1]
        fa_, fb_ = (br.surface_load(x.elem_kind, x.vertices, x.connectivity, cells, lfs, w, p, d, pressure=[1.5]) for x in (a, b))
        assert np.array_equal(fa_, fb_)


# --------------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", KINDS)
def test_surface_load_against_long_double(name):
    m = _distorted(name)
    cells, lfs = _face_subset(m, 0)
    w, p = br.face_rule(br.FACE_KIND[m.elem_kind], _rule_points(name))
    eng = fa.Engine()
    eng.set_mesh(m)
    rng = np.random.default_rng(11)
    x = eng.physical_face_quadrature_points(cells, lfs, p)
    xr = br.face_points(m.elem_kind, m.vertices, m.connectivity, cells, lfs, p)
    assert np.abs(x - xr).max() <= 1e-14
    for label, kind, s, data, count in _cases(m, cells, len(w), 0):
        ref = _reference(m, cells, lfs, w, p, kind, s, data)
        scale = float(np.abs(ref).max())
        garbage = scale * rng.uniform(-1, 1, s * m.num_nodes())        # out is accumulated into
        out = garbage.copy()
        eng.assemble_surface_load(out, kind, s, cells, lfs, w, p, data, count)
        err = float(np.abs((out.astype(np.longdouble) - garbage) - ref).max()) / scale
        print(f"{name} {label}: max|f| {scale:.3e} rel.err {err:.2e}")
        assert err <= TOL, (name, label, err)
        touched = np.zeros(m.num_nodes(), dtype=bool)
        for c, f in zip(cells, lfs):
            touched[m.connectivity[int(c)][br.FACES[m.elem_kind][int(f)]].astype(np.int64)] = True
        assert np.array_equal(out.reshape(-1, s)[~touched], garbage.reshape(-1, s)[~touched])   # only the faces' own nodes
        again = garbage.copy()
        eng.assemble_surface_load(again, kind, s, cells, lfs, w, p, data, count)
        assert np.array_equal(out, again)                              # two calls: bit for bit


@pytest.mark.gpu
def test_device_tensors_and_python_mirror():
    import torch

    m = _distorted("hex27")
    bf = m.find_boundary_faces()
    top = bf.select(lambda c, n: n[:, 2] > 0.5)
    assert 0 < len(top) < len(bf)
    rule = br.face_rule("quad9", 4)
    sl = fa.SurfaceLoad(m, top, rule).with_pressure(lambda x: 1.0 + x[..., 0] * x[..., 1])
    f = sl.assemble_vector()
    xq = br.face_points(m.elem_kind, m.vertices, m.connectivity, top.cells, top.local_faces, rule[1])
    ref = br.surface_load(m.elem_kind, m.vertices, m.connectivity, top.cells, top.local_faces, rule[0], rule[1], 3,
                          pressure=(1.0 + xq[..., 0] * xq[..., 1]).reshape(-1))
    assert float(np.abs(f - ref).max()) <= TOL * float(np.abs(ref).max())
    out_t = torch.zeros(3 * m.num_nodes(), dtype=torch.float64, device="cuda")
    sl.assemble_vector_into(out_t)
    assert np.array_equal(out_t.cpu().numpy(), f)                      # host and device forms: the same bits
    fa.VectorAssembler().assemble_vector_into(out_t, sl)               # accumulates: twice the load
    assert np.array_equal(out_t.cpu().numpy(), f + f)
    t = fa.SurfaceLoad(m, top, rule).with_traction(np.array([0.0, 0.0, -2.0])).assemble_vector()
    reft = br.surface_load(m.elem_kind, m.vertices, m.connectivity, top.cells, top.local_faces, rule[0], rule[1], 3, traction=[0, 0, -2.0])
    assert float(np.abs(t - reft).max()) <= TOL * float(np.abs(reft).max())


@pytest.mark.gpu
def test_bad_arguments():
    m = _linear("hex", 2)
    eng = fa.Engine()
    eng.set_mesh(m)
    w, p = br.face_rule("quad4", 2)
    out = np.zeros(3 * m.num_nodes())
    for cells, lfs in (([8], [0]), ([0], [6])):                       # cell / local face out of range
        with pytest.raises(fa.FenrisError) as e:
            eng.assemble_surface_load(out, _ffi.LOAD_PRESSURE, 3, np.array(cells, dtype=np.uint64), np.array(lfs, dtype=np.uint32), w, p, [1.0], 1)
        assert e.value.code == _ffi.FH_BAD_ARGUMENT
    with pytest.raises(fa.FenrisError):                                # a pressure needs s == d
        eng.assemble_surface_load(np.zeros(m.num_nodes()), _ffi.LOAD_PRESSURE, 1, np.array([0], dtype=np.uint64), np.array([0], dtype=np.uint32), w, p, [1.0], 1)
    with pytest.raises(fa.FenrisError):                                # data count that is none of 1, F, F nq
        eng.assemble_surface_load(out, _ffi.LOAD_PRESSURE, 3, np.array([0, 1], dtype=np.uint64), np.array([0, 0], dtype=np.uint32), w, p, [1.0] * 3, 3)
    assert np.all(out == 0.0)
    t20 = fa.tet20_mesh_from_tet4(_linear("tet", 1))
    eng.set_mesh(t20)
    with pytest.raises(fa.FenrisError) as e:
        eng.assemble_surface_load(np.zeros(3 * t20.num_nodes()), _ffi.LOAD_PRESSURE, 3, np.array([0], dtype=np.uint64), np.array([0], dtype=np.uint32),
                                  *br.face_rule("tri3", 2), [1.0], 1)
    assert e.value.code == _ffi.FH_UNSUPPORTED


def _interior_perturbed(m, n, seed=3):
    rng = np.random.default_rng(seed)
    v = m.vertices.copy()
    inside = ((v > 1e-12) & (v < 1 - 1e-12)).all(axis=1)
    v[inside] += (0.15 / n) * rng.uniform(-1, 1, (int(inside.sum()), v.shape[1]))
    return fa.Mesh(v, m.connectivity, m.elem_kind)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hex", "tet", "hex27", "quad"])
def test_divergence_theorem_patch(name):
    """u = A x on the box, interior vertices moved, boundary planar: the residual r(u) = int sigma : grad v of linear elasticity equals
    the surface load of the traction sigma n, node by node"""
    n = 3
    lin = _interior_perturbed(_linear(_BASE.get(name, name), n), n)
    m = _RAISE[name](lin) if name in _BASE else lin
    d = m.vertices.shape[1]
    A = np.array([[0.02, 0.01, -0.015], [0.005, -0.01, 0.02], [0.01, 0.015, 0.025]])[:d, :d]
    u = (m.vertices @ A.T).reshape(-1)
    lame = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e3, 0.3))
    mu, lam = lame.as_pair()
    eps = 0.5 * (A + A.T)
    sigma = 2 * mu * eps + lam * np.trace(eps) * np.eye(d)
    rule = {"hex": quadrature.tensor.hexahedron_gauss(2), "hex27": quadrature.tensor.hexahedron_gauss(3),
            "tet": quadrature.total_order.tetrahedron(2), "quad": quadrature.tensor.quadrilateral_gauss(2)}[name]
    asm = (fa.ElementEllipticAssemblerBuilder().with_finite_element_space(m)
           .with_operator(fa.MaterialEllipticOperator(fa.LinearElasticMaterial()))
           .with_quadrature_table(fa.UniformQuadratureTable.from_points_and_weights(rule[1], rule[0]).with_uniform_data(lame))
           .with_u(u).build())
    r = fa.VectorAssembler().assemble_vector(asm)
    bf = m.find_boundary_faces()
    A_, _, _ = br.face_area_vectors(m.elem_kind, m.vertices, m.connectivity, bf.cells, bf.local_faces)
    nrm = (A_ / np.sqrt(np.sum(A_ * A_, axis=1, keepdims=True))).astype(np.float64)
    traction = nrm @ sigma.T                                           # per face: sigma n
    f = fa.SurfaceLoad(m, bf, br.face_rule(br.FACE_KIND[m.elem_kind], 3)).with_traction(traction).assemble_vector()
    err = float(np.abs(r - f).max() / np.abs(r).max())
    print(f"patch {name}: max|r| {np.abs(r).max():.3e} rel.err {err:.2e}")
    assert err <= TOL


@pytest.mark.gpu
def test_closed_surface_identities():
    m = fa.io.load_msh_from_file(os.path.join(ROOT, "tests", "golden", "msh", "sphere_tet4_593.msh"), fa.TET4)
    bf = m.find_boundary_faces()
    rule = br.face_rule("tri3", 2)
    pr = 3.5
    f = fa.SurfaceLoad(m, bf, rule).with_pressure(pr).assemble_vector().reshape(-1, 3)
    A_, _, _ = br.face_area_vectors(m.elem_kind, m.vertices, m.connectivity, bf.cells, bf.local_faces)
    area = float(np.sum(np.sqrt(np.sum(A_ * A_, axis=1))))
    force, moment = f.sum(axis=0), np.cross(m.vertices, f).sum(axis=0)
    print(f"sphere: area {area:.6f} |force| {np.abs(force).max():.2e} |moment| {np.abs(moment).max():.2e}")
    assert np.abs(force).max() <= TOL * pr * area and np.abs(moment).max() <= TOL * pr * area
    # uniform traction on the face x = 1 of the unit box: the nodal forces sum to t (area 1)
    box = _linear("hex", 4)
    right = box.find_boundary_faces().select(lambda c, n: n[:, 0] > 0.5)
    assert len(right) == 16
    t = np.array([0.3, -1.25, 2.0])
    g = fa.SurfaceLoad(box, right, br.face_rule("quad4", 2)).with_traction(t).assemble_vector().reshape(-1, 3)
    assert np.abs(g.sum(axis=0) - t).max() <= 4 * np.finfo(float).eps * np.abs(t).max()
    assert np.all(g[box.vertices[:, 0] != 1.0] == 0.0)


@pytest.mark.gpu
def test_newton_bar_clamped_and_pressed():
    """NeoHookean Hex8 bar: clamp the boundary vertices at x = 0, press on the end x = L, solve; r(u) - f vanishes on the free dofs"""
    m = P.create_rectangular_uniform_hex_mesh(0.25, 8, 1, 1, 2)       # 2 x 0.25 x 0.25, 16 x 2 x 2 cells
    L = float(m.vertices[:, 0].max())
    bv = m.find_boundary_vertices()
    clamped = bv[m.vertices[bv.astype(np.int64), 0] == 0.0]
    assert len(clamped) == 9
    end = m.find_boundary_faces().select(lambda c, n: c[:, 0] > L - 1e-9)
    assert len(end) == 4
    f = fa.SurfaceLoad(m, end, br.face_rule("quad4", 2)).with_pressure(-20.0).assemble_vector()   # negative: pulls along +x
    assert abs(f.reshape(-1, 3)[:, 0].sum() - 20.0 * 0.0625) < 1e-13
    lame = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e3, 0.3))
    w, p = quadrature.tensor.hexahedron_gauss(2)
    u = np.zeros(3 * m.num_nodes())
    asm = (fa.ElementEllipticAssemblerBuilder().with_finite_element_space(m)
           .with_operator(fa.MaterialEllipticOperator(fa.NeoHookeanMaterial()))
           .with_quadrature_table(fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(lame)).with_u(u).build())
    tol = 1e-9
    res = fa.MatrixFreeNewton(asm).with_dirichlet_nodes(clamped).with_load(f).solve(u, fa.NewtonSettings(max_iterations=50, tolerance=tol))
    assert res.residual_norm <= tol and res.iterations >= 2
    asm.engine.set_u(u)
    r = fa.VectorAssembler().assemble_vector(asm)
    free = np.ones(m.num_nodes(), dtype=bool)
    free[clamped.astype(np.int64)] = False
    resid = (r - f).reshape(-1, 3)[free]
    print(f"newton: {res.iterations} iterations, |F| {res.residual_norm:.2e}, free residual {np.linalg.norm(resid):.2e}, tip u_x {u.reshape(-1, 3)[:, 0].max():.4e}")
    assert np.linalg.norm(resid) <= tol
    assert u.reshape(-1, 3)[:, 0].max() > 1e-3 and np.all(u.reshape(-1, 3)[clamped.astype(np.int64)] == 0.0)
