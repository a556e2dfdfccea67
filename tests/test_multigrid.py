"""Geometric multigrid (fh_mg_*, FH_PRECOND_MULTIGRID, fa.GeometricMultigrid): one V-cycle against a NumPy V-cycle on the oracle's
assembled matrices and the documented Chebyshev recurrence, symmetry, positivity, bitwise repeats, Dirichlet rows; MG-PCG iteration counts
that stay flat under refinement; tangent, shifted and Newton solves; the error contract."""
import numpy as np
import pytest
import scipy.sparse as sp

import fenris_amd as fa
from fenris_amd import _ffi, quadrature

FH_BAD_ARGUMENT, FH_INVALID_STATE, FH_UNSUPPORTED = 2, 5, 6
W, P = quadrature.tensor.hexahedron_gauss(2)
OPS = {"laplace": fa.LaplaceOperator(), "elastic": fa.MaterialEllipticOperator(fa.LinearElasticMaterial()),
       "neo_hookean": fa.MaterialEllipticOperator(fa.NeoHookeanMaterial())}


def _lame(nu=0.3):
    return fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, nu))


@pytest.fixture()
def engine():
    eng = fa.Engine(0)
    yield eng
    eng.close()


def _hierarchy(base, levels):
    """meshes (coarsest first, the fine one last) and their transfers"""
    return fa.refine_uniformly_repeat_with_transfers(fa.procedural.create_unit_box_uniform_hex_mesh_3d(base), levels)


def _assembler(engine, m, op, nu=0.3, u=None):
    s = 1 if op == "laplace" else 3
    qt = fa.UniformQuadratureTable.from_points_and_weights(P, W)
    qt = qt if op == "laplace" else qt.with_uniform_data(_lame(nu))
    return (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(m).with_operator(OPS[op]).with_quadrature_table(qt)
            .with_u(np.zeros(s * m.num_nodes()) if u is None else u).build())


def _clamp(m):
    return np.where(np.isclose(m.vertices[:, 0], 0.0))[0].astype(np.uint64)


def _dofs(nodes, s):
    return (s * np.asarray(nodes, dtype=np.int64)[:, None] + np.arange(s)).ravel()


def _oracle_matrix(m, op, nu, u, alpha, beta, rho):
    from oracle import oracle

    kind = {"laplace": oracle.LAPLACE, "elastic": oracle.LINEAR_ELASTIC, "neo_hookean": oracle.NEO_HOOKEAN}[op]
    params = None if op == "laplace" else _lame(nu).as_pair()
    A = 0
    if beta != 0.0:
        a = oracle.ElementAssembler(oracle.HEX8, kind, m.vertices, m.connectivity, W, P, params=params, u=u)
        st, _, ro, ci, v = oracle.assemble(a)
        assert st == 0
        A = beta * sp.csr_matrix((v, ci.astype(np.int64), ro.astype(np.int64)))
    if alpha != 0.0:
        a = oracle.ElementAssembler(oracle.HEX8, oracle.MASS_SCALAR if op == "laplace" else oracle.MASS_VECTOR, m.vertices, m.connectivity,
                                    W, P, params=(rho, 0.0))
        st, _, ro, ci, v = oracle.assemble(a)
        assert st == 0
        A = A + alpha * sp.csr_matrix((v, ci.astype(np.int64), ro.astype(np.int64)))
    return A.toarray()


def _injection(t):
    off = t.offsets.astype(np.int64)
    single = np.where(np.diff(off) == 1)[0]
    inj = np.full(t.num_coarse, -1, dtype=np.int64)
    inj[t.indices[off[single]].astype(np.int64)] = single
    return inj


def _np_vcycle(mg, meshes, transfers, op, nu, u_fine, clamp, alpha, beta, rho, r, coarse_op=None, degree=3, rng_=15.0):
    """the V-cycle of fh_mg_apply_dev restated on the oracle's matrices: Dirichlet rows and columns replaced by the device's scale"""
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
        o = op if (k == L or coarse_op is None) else coarse_op
        A = _oracle_matrix(meshes[k], o, nu, us[k].ravel() if o == "neo_hookean" else None, alpha, beta, rho)
        eng = mg.engine if k == L else mg.levels[k].engine
        import torch

        d = torch.empty(A.shape[0], dtype=torch.float64, device="cuda:0")
        eng.shifted_tangent_diagonal_dev(alpha, beta, d) if alpha != 0.0 else eng.tangent_diagonal_dev(d)
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


def _setup(engine, op, nu=0.3, coarse_operator="tangent", base=2, levels=2, u_amp=0.0):
    meshes, ts = _hierarchy(base, levels)
    fine = meshes[-1]
    s = 1 if op == "laplace" else 3
    u = np.zeros((fine.num_nodes(), s))
    if u_amp:
        u[:] = u_amp * np.sin(np.pi * fine.vertices[:, [0]])
    asm = _assembler(engine, fine, op, nu, u.ravel())
    mg = fa.GeometricMultigrid(asm, meshes[:-1], ts, coarse_operator=coarse_operator)
    return meshes, ts, asm, mg, u.ravel()


CASES = [("laplace", "tangent", 0.0, 1.0), ("elastic", "tangent", 0.0, 1.0), ("neo_hookean", "tangent", 0.0, 1.0),
         ("neo_hookean", "linearized", 0.0, 1.0), ("elastic", "tangent", 1.0, 1e-4), ("neo_hookean", "tangent", 1.0, 1e-4)]


@pytest.mark.gpu
@pytest.mark.parametrize("op,coarse,alpha,beta", CASES)
def test_vcycle_matches_numpy(engine, op, coarse, alpha, beta):
    import torch

    meshes, ts, asm, mg, u = _setup(engine, op, coarse_operator=coarse, u_amp=0.02 if op == "neo_hookean" else 0.0)
    clamp = _clamp(meshes[-1])
    rho = 1000.0 if alpha else None
    if rho is not None:
        for lv in mg.levels:
            lv.engine.set_mass_density(rho)
        engine.set_mass_density(rho)
    rng = np.random.default_rng(0)
    r = rng.standard_normal(len(u))
    z = torch.empty(len(u), dtype=torch.float64, device="cuda:0")
    mg.apply(torch.from_numpy(r).cuda(), z, alpha, beta, dirichlet_nodes=clamp, density=rho)
    zn = z.cpu().numpy()
    ref = _np_vcycle(mg, meshes, ts, op, 0.3, u, clamp, alpha, beta, rho or 0.0, r,
                     coarse_op="elastic" if coarse == "linearized" else None)
    assert np.abs(zn - ref).max() <= 1e-10 * np.abs(ref).max()
    lam = [mg.level_info(k)[0] for k in range(len(meshes))]
    assert all(1.0 <= x < 10.0 for x in lam[1:])


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["elastic", "neo_hookean"])
def test_vcycle_symmetric_positive_repeatable(engine, op):
    import torch

    meshes, ts, asm, mg, u = _setup(engine, op, u_amp=0.02 if op == "neo_hookean" else 0.0)
    clamp = _clamp(meshes[-1])
    rng = np.random.default_rng(1)
    n = len(u)
    r1, r2 = (torch.from_numpy(rng.standard_normal(n)).cuda() for _ in range(2))
    z1, z2, z1b = (torch.empty(n, dtype=torch.float64, device="cuda:0") for _ in range(3))
    mg.apply(r1, z1, dirichlet_nodes=clamp)
    mg.apply(r2, z2, dirichlet_nodes=clamp)
    mg.apply(r1, z1b, dirichlet_nodes=clamp)
    assert torch.equal(z1, z1b)
    a, b = float(torch.dot(z1, r2)), float(torch.dot(r1, z2))
    assert abs(a - b) <= 1e-12 * max(abs(a), abs(b))
    assert float(torch.dot(r1, z1)) > 0.0 and float(torch.dot(r2, z2)) > 0.0
    # Dirichlet rows: r / scale
    d = torch.empty(n, dtype=torch.float64, device="cuda:0")
    engine.tangent_diagonal_dev(d)
    dd = torch.from_numpy(_dofs(clamp, 3)).cuda()
    assert torch.equal(z1[dd], r1[dd] / d[dd])


@pytest.mark.gpu
def test_mg_pcg_iterations_stay_flat(engine):
    its_mg, its_j = [], []
    for levels in (2, 3, 4):   # 8^3, 16^3, 32^3 fine levels from 2^3
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
    # (rel_tol 1e-10: a few more iterations than at 1e-8)
    assert max(its_mg) <= 20 and max(its_mg) - min(its_mg) <= 2, its_mg
    assert its_j[1] >= 1.6 * its_j[0] and its_j[2] >= 1.6 * its_j[1], its_j


@pytest.mark.gpu
def test_mg_pcg_at_default_tolerance(engine):
    for levels in (2, 3):
        meshes, ts = _hierarchy(2, levels)
        fine = meshes[-1]
        asm = _assembler(engine, fine, "elastic")
        clamp = _clamp(fine)
        b = np.zeros(3 * fine.num_nodes())
        b[1::3] = -1.0
        b[_dofs(clamp, 3)] = 0.0
        mg = fa.GeometricMultigrid(asm, meshes[:-1], ts)
        x = np.zeros_like(b)
        it = fa.MatrixFreeOperator(asm).with_dirichlet_nodes(clamp).with_multigrid(mg).cg_solve(b, x, rel_tol=1e-8)
        assert it <= 15


@pytest.mark.gpu
@pytest.mark.parametrize("coarse", ["tangent", "linearized"])
def test_tangent_and_shifted_solves(engine, coarse):
    meshes, ts, asm, mg, u = _setup(engine, "neo_hookean", coarse_operator=coarse, levels=3, u_amp=0.02)
    clamp = _clamp(meshes[-1])
    rng = np.random.default_rng(3)
    b = rng.standard_normal(len(u))
    b[_dofs(clamp, 3)] = 0.0
    tan = fa.MatrixFreeTangent(asm).with_dirichlet_nodes(clamp).with_multigrid(mg)
    x_mg, x_j = np.zeros_like(b), np.zeros_like(b)
    it_mg = tan.cg_solve(b, x_mg, rel_tol=1e-10)
    it_j = tan.cg_solve(b, x_j, fa.PRECOND_JACOBI, rel_tol=1e-10)
    assert it_mg < it_j / 3
    assert np.abs(x_mg - x_j).max() <= 1e-7 * np.abs(x_j).max()
    sh = fa.MatrixFreeShiftedTangent(asm, 1000.0, 1.0, 1e-4).with_dirichlet_nodes(clamp).with_multigrid(mg)
    y_mg, y_j = np.zeros_like(b), np.zeros_like(b)
    it_mg = sh.cg_solve(b, y_mg, rel_tol=1e-10)
    it_j = sh.cg_solve(b, y_j, fa.PRECOND_JACOBI, rel_tol=1e-10)
    assert it_mg <= it_j
    assert np.abs(y_mg - y_j).max() <= 1e-7 * np.abs(y_j).max()


@pytest.mark.gpu
def test_newton_with_multigrid_matches_jacobi():
    meshes, ts = _hierarchy(1, 2)
    fine = meshes[-1]
    clamp = _clamp(fine)
    face = np.where(np.isclose(fine.vertices[:, 0], 1.0))[0]
    f = np.zeros(3 * fine.num_nodes())
    f[3 * face] = 2e5 / len(face)
    tol = 1e-8 * np.linalg.norm(f)
    out = []
    for use_mg in (False, True):
        eng = fa.Engine(0)
        asm = _assembler(eng, fine, "neo_hookean")
        newton = fa.MatrixFreeNewton(asm).with_dirichlet_nodes(clamp).with_load(f)
        mg = None
        if use_mg:
            mg = fa.GeometricMultigrid(asm, meshes[:-1], ts)
            newton.with_multigrid(mg)
        u = np.zeros_like(f)
        res = newton.solve(u, fa.NewtonSettings(60, tol), linear_rel_tol=1e-12)
        out.append((res, u.copy()))
        del mg
        eng.close()
    (rj, uj), (rm, um) = out
    assert (rm.iterations, rm.residual_evaluations) == (rj.iterations, rj.residual_evaluations)
    assert rm.linear_iterations < rj.linear_iterations
    assert np.abs(um - uj).max() <= 1e-8 * np.abs(uj).max()


@pytest.mark.gpu
def test_errors(engine):
    meshes, ts, asm, mg, u = _setup(engine, "elastic")
    clamp = _clamp(meshes[-1])
    b = np.ones(len(u))
    b[_dofs(clamp, 3)] = 0.0
    op = fa.MatrixFreeOperator(asm).with_dirichlet_nodes(clamp)
    with pytest.raises(_ffi.FenrisError) as e:
        op.cg_solve(b, np.zeros_like(b), fa.PRECOND_MULTIGRID)
    assert e.value.code == FH_INVALID_STATE
    mg._bind(clamp)
    # a coarse Dirichlet set that does not follow the injection
    mg.levels[0].engine.set_operator_dirichlet_nodes(np.array([0], dtype=np.uint64))
    mg._destroy()
    with pytest.raises(_ffi.FenrisError) as e:
        mg._create()
    assert e.value.code == FH_BAD_ARGUMENT
    # a coarse node without its injected fine copy
    mg._key = None
    mg._bind(clamp)
    mg._destroy()
    t = ts[-1]
    bad = fa.Transfer(t.offsets.copy(), t.indices.copy(), t.weights.copy(), t.num_coarse)
    bad.weights[0] = 0.999
    mg.transfers[-1] = bad
    with pytest.raises(_ffi.FenrisError) as e:
        mg._create()
    assert e.value.code == FH_BAD_ARGUMENT


@pytest.mark.gpu
def test_coarsest_over_4096_dofs_unsupported(engine):
    meshes, ts = _hierarchy(11, 1)   # 12^3 nodes, 3 dofs each
    asm = _assembler(engine, meshes[-1], "elastic")
    mg = fa.GeometricMultigrid(asm, meshes[:-1], ts)
    with pytest.raises(_ffi.FenrisError) as e:
        mg._bind(_clamp(meshes[-1]))
    assert e.value.code == FH_UNSUPPORTED


@pytest.mark.gpu
def test_indefinite_coarse_tangent(engine):
    """NeoHookean nu 0.45 at u = 0.02 sin(pi X): the coarse tangents are not SPD (checked on the oracle), the linearized ones are"""
    meshes, ts, asm, mg, u = _setup(engine, "neo_hookean", nu=0.45, levels=3, u_amp=0.02)
    clamp = _clamp(meshes[-1])
    b = np.ones(len(u))
    b[_dofs(clamp, 3)] = 0.0
    tan = fa.MatrixFreeTangent(asm).with_dirichlet_nodes(clamp).with_multigrid(mg)
    with pytest.raises(fa.CgSolveError) as e:
        tan.cg_solve(b, np.zeros_like(b), rel_tol=1e-8)
    assert e.value.code == _ffi.FH_CG_INDEFINITE_PRECONDITIONER
    newton = fa.MatrixFreeNewton(asm).with_dirichlet_nodes(clamp).with_multigrid(mg)
    with pytest.raises(fa.JacobianError) as e:
        newton.solve(u.copy(), fa.NewtonSettings(5, 1e-12))
    assert e.value.code == _ffi.FH_NEWTON_JACOBIAN_ERROR and e.value.cg_code == _ffi.FH_CG_INDEFINITE_PRECONDITIONER
