"""The matrix-free LOBPCG eigensolver (fh_eigs_lowest, MatrixFreeEigensolver) against the dense spectrum: K and M assembled with the
existing assemblers on the same mesh, table and density, the free-dof submatrices taken in numpy, lambda = eigh(L^-1 K_ff L^-T) with
L = cholesky(M_ff).

Per case, with x_i the returned vectors on the free dofs, theta_i the returned values and r_i = K_ff x_i - theta_i M_ff x_i recomputed in numpy:
  - ||r_i||_2 <= tol (|theta_i| + shift) ||M x_i||_2 + nnz_row_max eps (|| |K||x_i| ||_2 + |theta_i| || |M||x_i| ||_2): the solver's criterion plus
    the rounding of the recomputation (a row of K x is an inner product of at most nnz_row_max terms);
  - |theta_i - lambda_i| <= ||r_i||_2 / sqrt(lambda_min(M_ff)) for the i-th sorted pair: |lambda - theta| <= ||r||_{M^-1} for an M-normalised x
    (Parlett, The Symmetric Eigenvalue Problem, 15.9.1), and ||r||_{M^-1} <= ||r||_2 / sqrt(lambda_min(M)).  A missed mode fails it,
    because m never cuts a cluster: (lambda_{m+1} - lambda_m) >= 0.05 lambda_{m+1} is asserted from the dense spectrum first;
  - ||X^T M X - I||_max <= tol, and X exactly zero on the Dirichlet dofs.
m is the first count at or above the case's nominal one at which the gap condition holds."""
import ctypes as C

import numpy as np
import pytest

import fenris_amd as fa
from fenris_amd import _ffi, quadrature

EPS = np.finfo(float).eps
TOL = 1e-8
RHO = 2.0
LAME = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e3, 0.3))
FH_BAD_ARGUMENT, FH_INVALID_STATE, FH_UNSUPPORTED, FH_EIG_MAX_ITERATIONS = 2, 5, 6, 13


def _dense(csr):
    ro, ci = np.asarray(csr.row_offsets, dtype=np.int64), np.asarray(csr.col_indices, dtype=np.int64)
    v = csr.values.cpu().numpy() if hasattr(csr.values, "cpu") else np.asarray(csr.values)
    a = np.zeros((len(ro) - 1, len(ro) - 1))
    a[np.repeat(np.arange(len(ro) - 1), np.diff(ro)), ci] = v
    return a


class Case:
    """one problem: the assembler on its engine, the dense K and M, the free dofs and the dense spectrum on them"""

    def __init__(self, mesh, op, wp, s, clamp, u=None):
        w, p = (np.asarray(a) for a in wp)
        self.mesh, self.s, self.clamp = mesh, s, clamp
        self.engine, self.meng = fa.Engine(0), fa.Engine(0)
        qt = fa.UniformQuadratureTable.from_points_and_weights(p, w)
        self.n = s * mesh.num_nodes()
        self.asm = (fa.ElementEllipticAssemblerBuilder(self.engine).with_finite_element_space(mesh).with_operator(op)
                    .with_quadrature_table(qt if s == 1 else qt.with_uniform_data(LAME)).with_u(np.zeros(self.n) if u is None else u).build())
        masm = (fa.ElementMassAssembler.with_solution_dim(s, self.meng).with_space(mesh)
                .with_quadrature_table(fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(fa.Density(RHO))))
        kc = fa.CsrAssembler(fa.SCATTER_GATHER).assemble(self.asm)
        self.nnz_row_max = int(np.diff(np.asarray(kc.row_offsets, dtype=np.int64)).max())
        self.K, self.M = _dense(kc), _dense(fa.CsrAssembler(fa.SCATTER_GATHER).assemble(masm))
        fixed = np.zeros(self.n, dtype=bool)
        if clamp is not None and len(clamp):
            fixed[(np.asarray(clamp, dtype=np.int64)[:, None] * s + np.arange(s)).ravel()] = True
        self.fixed, self.free = fixed, np.where(~fixed)[0]
        self.Kf, self.Mf = self.K[np.ix_(self.free, self.free)], self.M[np.ix_(self.free, self.free)]
        self.Kf, self.Mf = 0.5 * (self.Kf + self.Kf.T), 0.5 * (self.Mf + self.Mf.T)
        low = np.linalg.cholesky(self.Mf)
        h = np.linalg.solve(low, np.linalg.solve(low, self.Kf).T).T
        self.lam, v = np.linalg.eigh(0.5 * (h + h.T))
        self.phi = np.linalg.solve(low.T, v)            # M-orthonormal dense vectors on the free dofs
        self.m_min = np.linalg.eigvalsh(self.Mf)[0]

    def close(self):
        self.engine.close()
        self.meng.close()

    def modes(self, nominal):
        """the first m >= nominal that does not cut a cluster (asserted: found within 8 of it)"""
        for m in range(nominal, nominal + 9):
            if self.lam[m] - self.lam[m - 1] >= 0.05 * self.lam[m]:
                return m
        raise AssertionError("no gap in the dense spectrum near m = %d: %r" % (nominal, self.lam[nominal - 1:nominal + 9]))

    def solver(self, shift=0.0):
        return fa.MatrixFreeEigensolver(self.asm, RHO).with_dirichlet_nodes(self.clamp).with_shift(shift)

    def check(self, res, m, shift=0.0, zero_modes=0, tol=TOL):
        assert self.lam[m] - self.lam[m - 1] >= 0.05 * self.lam[m]
        th, x = res.values, np.asarray(res.vectors)
        assert x.shape == (self.n, m) and np.all(np.diff(th) >= 0.0)
        assert np.all(x[self.fixed] == 0.0)
        xf = x[self.free]
        mx, kx = self.Mf @ xf, self.Kf @ xf
        r = np.linalg.norm(kx - mx * th, axis=0)
        rounding = self.nnz_row_max * EPS * (np.linalg.norm(np.abs(self.Kf) @ np.abs(xf), axis=0)
                                             + np.abs(th) * np.linalg.norm(np.abs(self.Mf) @ np.abs(xf), axis=0))
        crit = tol * (np.abs(th) + shift) * np.linalg.norm(mx, axis=0)
        print("residual / criterion:", np.array2string(r / crit, precision=3), " reported:", np.array2string(res.residual_norms / crit, precision=3))
        assert np.all(r <= crit + rounding), (r, crit, rounding)
        lam = self.lam[:m].copy()
        lam[:zero_modes] = 0.0
        err, ebound = np.abs(th - lam), r / np.sqrt(self.m_min)
        print("eigenvalue error / bound:", np.array2string(err / ebound, precision=3))
        assert np.all(err <= ebound), (th, lam, ebound)
        orth = np.abs(xf.T @ mx - np.eye(m)).max()
        assert orth <= tol, orth
        return r


def _cantilever_mesh():
    return fa.procedural.create_rectangular_uniform_hex_mesh(1.0, 3, 3, 8, 1)


def _end_face(mesh):
    z = mesh.vertices[:, 2]
    return np.where(z == z.min())[0].astype(np.uint64)


ELASTIC = lambda: fa.MaterialEllipticOperator(fa.LinearElasticMaterial())   # noqa: E731


@pytest.fixture(scope="module")
def cantilever():
    mesh = _cantilever_mesh()
    case = Case(mesh, ELASTIC(), quadrature.tensor.hexahedron_gauss(2), 3, _end_face(mesh))
    yield case
    case.close()


@pytest.fixture(scope="module")
def cantilever_solution(cantilever):
    m = cantilever.modes(6)
    return m, cantilever.solver().solve(m, tol=TOL, preconditioner=fa.PRECOND_JACOBI)


@pytest.mark.gpu
def test_clamped_cantilever(cantilever, cantilever_solution):
    m, res = cantilever_solution
    print("m =", m, "iterations", res.iterations, "applications", res.applications, "restarts", res.restarts)
    cantilever.check(res, m)


@pytest.mark.gpu
def test_free_body_tet4():
    mesh = fa.procedural.create_unit_box_uniform_tet_mesh_3d(2)
    case = Case(mesh, ELASTIC(), quadrature.total_order.tetrahedron(2), 3, None)
    try:
        m = case.modes(9)
        shift = float(case.lam[6])
        assert np.all(np.abs(case.lam[:6]) <= 1e-9 * case.lam[6])   # six rigid modes
        res = case.solver(shift).solve(m, tol=TOL, preconditioner=fa.PRECOND_JACOBI)
        print("m =", m, "iterations", res.iterations)
        case.check(res, m, shift=shift, zero_modes=6)
    finally:
        case.close()


@pytest.mark.gpu
def test_laplace_quad4_double_eigenvalues():
    mesh = fa.procedural.create_unit_square_uniform_quad_mesh_2d(9)
    v = mesh.vertices
    edge = np.where((v[:, 0] == v[:, 0].min()) | (v[:, 0] == v[:, 0].max()) | (v[:, 1] == v[:, 1].min()) | (v[:, 1] == v[:, 1].max()))[0]
    case = Case(mesh, fa.LaplaceOperator(), quadrature.tensor.quadrilateral_gauss(2), 1, edge.astype(np.uint64))
    try:
        m = case.modes(6)
        res = case.solver().solve(m, tol=TOL, preconditioner=fa.PRECOND_JACOBI)
        r = case.check(res, m)
        lam, xf = case.lam, np.asarray(res.vectors)[case.free]
        # Davis-Kahan: the computed vectors of each dense cluster span it
        i, doubles = 0, 0
        while i < m:
            j = i + 1
            while j < m and lam[j] - lam[i] <= 1e-8 * lam[j]:
                j += 1
            doubles += j - i > 1
            phi = case.phi[:, i:j]
            outside = np.concatenate([lam[:i], lam[j:]])
            for k in range(i, j):
                gap = np.abs(outside[:, None] - lam[i:j][None, :]).min()
                d = xf[:, k] - phi @ (phi.T @ (case.Mf @ xf[:, k]))
                dist = np.sqrt(d @ (case.Mf @ d))
                assert dist <= r[k] / (np.sqrt(case.m_min) * gap), (k, dist, r[k], gap)
            i = j
        assert doubles >= 1   # the case is about double eigenvalues
    finally:
        case.close()


@pytest.mark.gpu
def test_prestressed_neo_hookean():
    mesh = _cantilever_mesh()
    x = mesh.vertices
    u = np.zeros((mesh.num_nodes(), 3))
    u[:, 2] = 0.02 * x[:, 2] + 0.01 * np.sin(0.3 * x[:, 2])          # a small smooth stretch along the axis
    u[:, 0] = -0.004 * x[:, 0] * x[:, 2] / 8.0
    case = Case(mesh, fa.MaterialEllipticOperator(fa.NeoHookeanMaterial()), quadrature.tensor.hexahedron_gauss(2), 3, _end_face(mesh), u=u.ravel())
    try:
        m = case.modes(6)
        res = case.solver().solve(m, tol=TOL, preconditioner=fa.PRECOND_JACOBI)
        print("m =", m, "iterations", res.iterations)
        case.check(res, m)
    finally:
        case.close()


@pytest.mark.gpu
def test_multigrid_preconditioner():
    meshes, ts = fa.refine_uniformly_repeat_with_transfers(_cantilever_mesh(), 1)
    fine = meshes[-1]
    case = Case(fine, ELASTIC(), quadrature.tensor.hexahedron_gauss(2), 3, _end_face(fine))
    try:
        m = case.modes(6)
        mg = fa.GeometricMultigrid(case.asm, meshes[:-1], ts)
        res = case.solver().with_multigrid(mg).solve(m, tol=TOL)
        case.check(res, m)
        res_j = case.solver().solve(m, tol=TOL, preconditioner=fa.PRECOND_JACOBI)
        case.check(res_j, m)
        print("iterations: multigrid", res.iterations, "Jacobi", res_j.iterations)
        del mg
    finally:
        case.close()


@pytest.mark.gpu
def test_contract(cantilever, cantilever_solution):
    import torch

    m, res = cantilever_solution
    solver = cantilever.solver()
    again = solver.solve(m, tol=TOL, preconditioner=fa.PRECOND_JACOBI)
    assert np.array_equal(again.values, res.values) and np.array_equal(again.vectors, res.vectors)       # bit for bit
    assert (again.iterations, again.applications, again.restarts) == (res.iterations, res.applications, res.restarts)
    on_device = solver.solve(m, tol=TOL, preconditioner=fa.PRECOND_JACOBI, device=True)                   # the device entry point: the same bits
    assert torch.is_tensor(on_device.vectors)
    assert np.array_equal(on_device.values, res.values) and np.array_equal(on_device.vectors.cpu().numpy(), res.vectors)
    warm = solver.solve(m, tol=TOL, preconditioner=fa.PRECOND_JACOBI, guess=res.vectors)
    assert warm.iterations == 0
    cantilever.check(warm, m)
    # max_iter: the partial pairs are Rayleigh quotients of the returned X
    with pytest.raises(fa.EigenSolveError) as ei:
        solver.solve(m, tol=TOL, max_iter=2, preconditioner=fa.PRECOND_JACOBI)
    assert ei.value.code == FH_EIG_MAX_ITERATIONS and ei.value.result.iterations == 2
    part = ei.value.result
    xf = part.vectors[cantilever.free]
    n = len(cantilever.free)
    kq = np.einsum("ij,ij->j", xf, cantilever.Kf @ xf)
    mq = np.einsum("ij,ij->j", xf, cantilever.Mf @ xf)
    allowed = n * EPS * (np.einsum("ij,ij->j", np.abs(xf), np.abs(cantilever.Kf) @ np.abs(xf))
                         + np.abs(part.values) * np.einsum("ij,ij->j", np.abs(xf), np.abs(cantilever.Mf) @ np.abs(xf)))
    print("Rayleigh quotient error / n eps bound:", np.array2string(np.abs(part.values * mq - kq) / allowed, precision=3))
    assert np.all(np.abs(part.values * mq - kq) <= allowed)
    assert np.all(part.vectors[cantilever.fixed] == 0.0)


@pytest.mark.gpu
def test_argument_errors(cantilever):
    solver = cantilever.solver()
    lib, h = cantilever.engine._lib, cantilever.engine._h
    n = cantilever.n
    x, th = np.zeros(40 * n), np.zeros(40)

    def call(m, shift=0.0, pre=1, tol=1e-8, handle=h, xx=x, tt=th):
        return lib.fh_eigs_lowest(handle, m, shift, pre, tol, 0, 0, _ffi.fp(xx) if xx is not None else None, _ffi.fp(tt) if tt is not None else None,
                                  None, None)

    solver._bind(force=True)
    assert call(0) == FH_BAD_ARGUMENT
    assert call(33) == FH_BAD_ARGUMENT
    assert call(4, shift=-1.0) == FH_BAD_ARGUMENT
    assert call(4, tol=float("nan")) == FH_BAD_ARGUMENT
    assert call(4, tol=float("inf")) == FH_BAD_ARGUMENT
    assert call(4, pre=7) == FH_BAD_ARGUMENT
    assert call(4, xx=None) == FH_BAD_ARGUMENT
    assert call(4, tt=None) == FH_BAD_ARGUMENT
    assert call(4, pre=fa.PRECOND_MULTIGRID) == FH_INVALID_STATE          # no hierarchy attached
    # m above a third of the free dofs: all but two nodes clamped leaves 6 free dofs
    cantilever.engine.set_operator_dirichlet_nodes(np.arange(2, cantilever.mesh.num_nodes(), dtype=np.uint64))
    assert call(3) == FH_BAD_ARGUMENT
    solver._bind(force=True)
    # no density
    mesh = cantilever.mesh
    w, p = (np.asarray(a) for a in quadrature.tensor.hexahedron_gauss(2))
    eng = fa.Engine(0)
    try:
        (fa.ElementEllipticAssemblerBuilder(eng).with_finite_element_space(mesh).with_operator(ELASTIC())
         .with_quadrature_table(fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(LAME)).with_u(np.zeros(n)).build())
        assert call(4, handle=eng._h) == FH_INVALID_STATE
    finally:
        eng.close()
    # the mass operators are not a stiffness
    assert call(4, handle=cantilever.meng._h) == FH_UNSUPPORTED
    with pytest.raises(ValueError):
        solver.solve(4, guess=np.zeros((n, 3)))
