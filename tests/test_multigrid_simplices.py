"""Geometric multigrid on tetrahedra: hierarchies from the device refiner (fh_refine_uniform), one V-cycle against a NumPy V-cycle on the
oracle's assembled Tet4 matrices, symmetry, positivity, bitwise repeats, and MG-PCG against Jacobi-PCG under refinement.  The NumPy
V-cycle restates the one of tests/test_multigrid.py, whose helpers assemble Hex8 matrices only."""
import numpy as np
import pytest
import scipy.sparse as sp

import fenris_amd as fa
from fenris_amd import quadrature

W, P = quadrature.total_order.tetrahedron(2)
OPS = {"laplace": fa.LaplaceOperator(), "elastic": fa.MaterialEllipticOperator(fa.LinearElasticMaterial()),
       "neo_hookean": fa.MaterialEllipticOperator(fa.NeoHookeanMaterial())}
LAME = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.3))


@pytest.fixture()
def engine():
    eng = fa.Engine(0)
    yield eng
    eng.close()


def _hierarchy(base, levels):
    """meshes (coarsest first) and transfers, refined on the device by an engine of their own"""
    eng = fa.Engine(0)
    try:
        return fa.refine_uniformly_repeat_with_transfers(fa.procedural.create_unit_box_uniform_tet_mesh_3d(base), levels, eng)
    finally:
        eng.close()


def _assembler(engine, m, op, u=None):
    s = 1 if op == "laplace" else 3
    qt = fa.UniformQuadratureTable.from_points_and_weights(P, W)
    qt = qt if op == "laplace" else qt.with_uniform_data(LAME)
    return (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(m).with_operator(OPS[op]).with_quadrature_table(qt)
            .with_u(np.zeros(s * m.num_nodes()) if u is None else u).build())


def _clamp(m):
    """the far face x = 1"""
    return np.where(np.isclose(m.vertices[:, 0], 1.0))[0].astype(np.uint64)


def _dofs(nodes, s):
    return (s * np.asarray(nodes, dtype=np.int64)[:, None] + np.arange(s)).ravel()


def _injection(t):
    off = t.offsets.astype(np.int64)
    single = np.where(np.diff(off) == 1)[0]
    inj = np.full(t.num_coarse, -1, dtype=np.int64)
    inj[t.indices[off[single]].astype(np.int64)] = single
    return inj


def _oracle_matrix(m, op, u):
    from oracle import oracle

    kind = {"laplace": oracle.LAPLACE, "elastic": oracle.LINEAR_ELASTIC, "neo_hookean": oracle.NEO_HOOKEAN}[op]
    a = oracle.ElementAssembler(oracle.TET4, kind, m.vertices, m.connectivity, W, P, params=None if op == "laplace" else LAME.as_pair(), u=u)
    st, _, ro, ci, v = oracle.assemble(a)
    assert st == 0
    return sp.csr_matrix((v, ci.astype(np.int64), ro.astype(np.int64))).toarray()


def _np_vcycle(mg, meshes, transfers, op, u_fine, clamp, r, degree=3, rng_=15.0):
    """the V-cycle of fh_mg_apply_dev on the oracle's matrices: Dirichlet rows and columns replaced by the device's scale, Chebyshev-Jacobi
    smoothing on [lambda / range, 1.1 lambda] with the device's lambda, exact coarsest solve"""
    import torch

    s = 1 if op == "laplace" else 3
    L = len(meshes) - 1
    masks, us = [None] * (L + 1), [None] * (L + 1)
    mask = np.zeros(meshes[-1].num_nodes(), dtype=bool)
    mask[clamp.astype(np.int64)] = True
    masks[L], us[L] = mask, u_fine.reshape(-1, s)
    for k in range(L - 1, -1, -1):
        inj = _injection(transfers[k])
        masks[k], us[k] = masks[k + 1][inj], us[k + 1][inj]
    As, Ps = [], []
    for k in range(L + 1):
        A = _oracle_matrix(meshes[k], op, us[k].ravel() if op == "neo_hookean" else None)
        eng = mg.engine if k == L else mg.levels[k].engine
        d = torch.empty(A.shape[0], dtype=torch.float64, device="cuda:0")
        eng.tangent_diagonal_dev(d)
        dd = _dofs(np.where(masks[k])[0], s)
        scale = d.cpu().numpy()[dd]
        A[dd, :] = 0.0
        A[:, dd] = 0.0
        A[dd, dd] = scale
        As.append(A)
        if k:
            Ps.append(sp.kron(transfers[k - 1].to_scipy(), sp.identity(s)).toarray())
    lam = [mg.level_info(k)[0] for k in range(L + 1)]

    def cheb(k, b, x):
        A, D = As[k], np.diag(As[k])
        hi, lo = 1.1 * lam[k], lam[k] / rng_
        th, de = (hi + lo) / 2, (hi - lo) / 2
        if x is None:
            x, r_ = np.zeros_like(b), b.copy()
        else:
            r_ = b - A @ x
        d = r_ / D / th
        rho_ = de / th
        for j in range(1, degree + 1):
            x = x + d
            if j < degree:
                r_ = r_ - A @ d
                rho1 = 1.0 / (2 * th / de - rho_)
                d = rho1 * rho_ * d + (2 * rho1 / de) * (r_ / D)
                rho_ = rho1
        return x

    def vc(k, b):
        if k == 0:
            return np.linalg.solve(As[0], b)
        fd, cd = _dofs(np.where(masks[k])[0], s), _dofs(np.where(masks[k - 1])[0], s)
        x = cheb(k, b, None)
        res = b - As[k] @ x
        res[fd] = 0.0
        bc = Ps[k - 1].T @ res
        bc[cd] = 0.0
        corr = Ps[k - 1] @ vc(k - 1, bc)
        corr[fd] = 0.0
        x = cheb(k, b, x + corr)
        x[fd] = b[fd] / np.diag(As[k])[fd]
        return x

    return vc(L, r)


def _setup(engine, op):
    meshes, ts = _hierarchy(1, 2)    # BCC 1 -> 2 -> 4
    fine = meshes[-1]
    s = 1 if op == "laplace" else 3
    u = np.zeros((fine.num_nodes(), s))
    if op == "neo_hookean":
        u[:] = 0.02 * np.sin(np.pi * fine.vertices[:, [0]])
    asm = _assembler(engine, fine, op, u.ravel())
    return meshes, ts, asm, fa.GeometricMultigrid(asm, meshes[:-1], ts), u.ravel()


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["laplace", "elastic", "neo_hookean"])
def test_vcycle_on_tetrahedra(engine, op):
    import torch

    meshes, ts, asm, mg, u = _setup(engine, op)
    assert [m.num_elements() for m in meshes] == [12, 96, 768]
    clamp = _clamp(meshes[-1])
    rng = np.random.default_rng(0)
    n = len(u)
    r1, r2 = rng.standard_normal(n), rng.standard_normal(n)
    t1, t2 = torch.from_numpy(r1).cuda(), torch.from_numpy(r2).cuda()
    z1, z2, z1b = (torch.empty(n, dtype=torch.float64, device="cuda:0") for _ in range(3))
    mg.apply(t1, z1, dirichlet_nodes=clamp)
    mg.apply(t2, z2, dirichlet_nodes=clamp)
    mg.apply(t1, z1b, dirichlet_nodes=clamp)
    ref = _np_vcycle(mg, meshes, ts, op, u, clamp, r1)
    assert np.abs(z1.cpu().numpy() - ref).max() <= 1e-10 * np.abs(ref).max()
    assert torch.equal(z1, z1b)                                               # repeatable bit for bit
    a, b = float(torch.dot(z1, t2)), float(torch.dot(t1, z2))
    assert abs(a - b) <= 1e-12 * max(abs(a), abs(b))                          # symmetric
    assert float(torch.dot(t1, z1)) > 0.0 and float(torch.dot(t2, z2)) > 0.0  # positive


@pytest.mark.gpu
def test_mg_pcg_on_tetrahedra():
    its_mg, its_j = [], []
    for levels in (1, 2, 3):   # fine levels BCC 4, 8, 16 from the coarsest BCC 2 (105 dofs)
        meshes, ts = _hierarchy(2, levels)
        fine = meshes[-1]
        eng = fa.Engine(0)
        asm = _assembler(eng, fine, "elastic")
        clamp = _clamp(fine)
        b = np.zeros(3 * fine.num_nodes())
        b[1::3] = -1.0 / fine.num_nodes()
        b[_dofs(clamp, 3)] = 0.0
        mg = fa.GeometricMultigrid(asm, meshes[:-1], ts)
        op = fa.MatrixFreeOperator(asm).with_dirichlet_nodes(clamp).with_multigrid(mg)
        x_mg, x_j = np.zeros_like(b), np.zeros_like(b)
        its_mg.append(op.cg_solve(b, x_mg, rel_tol=1e-10))
        its_j.append(op.cg_solve(b, x_j, fa.PRECOND_JACOBI, rel_tol=1e-10))
        assert np.abs(x_mg - x_j).max() <= 1e-7 * np.abs(x_j).max()
        del mg
        eng.close()
    print(f"tet4 elastic, fine BCC 4 / 8 / 16 from BCC 2: MG-PCG iterations {its_mg}, Jacobi-PCG iterations {its_j}")
    assert meshes[0].num_nodes() * 3 == 105
    assert all(m < j / 2 for m, j in zip(its_mg, its_j)), (its_mg, its_j)
    assert its_mg[2] / its_mg[0] < 0.5 * its_j[2] / its_j[0], (its_mg, its_j)
