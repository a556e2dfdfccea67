"""Newton's method on the device (fh_newton_solve(_dev), MatrixFreeNewton): newton_line_search of fenris-optimize/src/newton.rs for
F(u) = alpha M (u - u_ref) + beta (r(u) - f), against a NumPy Newton with the same backtracking rule on the oracle's residual and assembled
tangent (dense solve on the free dofs), against fh_cg_solve_matrix_free for the linear operators, and against the mass and residual
assembled independently for the implicit step."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import fenris_amd as fa
from fenris_amd import _ffi, quadrature

LAME = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.3))
FH_BAD_ARGUMENT, FH_INVALID_STATE, FH_UNSUPPORTED = 2, 5, 6
OKIND = {"HEX8": 1, "TET4": 2, "QUAD4": 0, "TET10": 5}


@pytest.fixture()
def engine():
    eng = fa.Engine(0)
    yield eng
    eng.close()


def _mesh(kind, res=3):
    box3, tet3 = fa.procedural.create_unit_box_uniform_hex_mesh_3d, fa.procedural.create_unit_box_uniform_tet_mesh_3d
    make = {"HEX8": (lambda: box3(res), quadrature.tensor.hexahedron_gauss(2)),
            "TET4": (lambda: tet3(res), quadrature.total_order.tetrahedron(2)),
            "QUAD4": (lambda: fa.procedural.create_unit_square_uniform_quad_mesh_2d(res), quadrature.tensor.quadrilateral_gauss(2)),
            "TET10": (lambda: fa.tet10_mesh_from_tet4(tet3(2)), quadrature.total_order.tetrahedron(4))}
    gen, (w, p) = make[kind]
    return gen(), np.asarray(w), np.asarray(p)


def _operator(op):
    return {"laplace": fa.LaplaceOperator(), "elastic": fa.MaterialEllipticOperator(fa.LinearElasticMaterial()),
            "neo_hookean": fa.MaterialEllipticOperator(fa.NeoHookeanMaterial()), "stvk": fa.MaterialEllipticOperator(fa.StVKMaterial())}[op]


def _assembler(engine, m, w, p, op, u=None, qt=None):
    s = 1 if op == "laplace" else m.vertices.shape[1]
    if qt is None:
        qt = fa.UniformQuadratureTable.from_points_and_weights(p, w)
        qt = qt if op == "laplace" else qt.with_uniform_data(LAME)
    return (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(m).with_operator(_operator(op)).with_quadrature_table(qt)
            .with_u(np.zeros(s * m.num_nodes()) if u is None else u).build())


def _clamped_pull(m, load, s=None):
    """x = 0 clamped, a total force `load` along +x spread over the nodes of x = 1"""
    x = m.vertices
    s = s or x.shape[1]
    clamp = np.where(np.isclose(x[:, 0], 0.0))[0]
    face = np.where(np.isclose(x[:, 0], 1.0))[0]
    f = np.zeros(s * len(x))
    f[s * face] = load / len(face)
    return clamp, f


def _np_newton(oracle, kind, op, m, w, p, u0, f, dirichlet, tol, backtracking=True, max_it=60):
    """newton_line_search with BacktrackingLineSearch / NoLineSearch on the oracle: (status, u, iterations, evaluations, accepted steps)"""
    s = m.vertices.shape[1]
    okind, oop = OKIND[kind], {"neo_hookean": oracle.NEO_HOOKEAN, "stvk": oracle.STVK}[op]
    free = np.ones(s * m.num_nodes(), dtype=bool)
    for k in range(s):
        free[s * np.asarray(dirichlet, dtype=np.int64) + k] = False

    def residual(u):
        asm = oracle.ElementAssembler(okind, oop, m.vertices, m.connectivity, w, p, params=LAME.as_pair(), u=u)
        st, _, r = oracle.assemble_vector(asm)
        assert st == 0
        F = r - f
        F[~free] = 0.0
        return F, asm

    u = u0.copy()
    F, asm = residual(u)
    it, evals, steps = 0, 1, []
    while True:
        fn = np.linalg.norm(F)
        if not np.isfinite(fn):
            return "nonfinite", u, it, evals, steps
        if fn <= tol:
            return "ok", u, it, evals, steps
        if it == max_it:
            return "maxit", u, it, evals, steps
        _, _, ro, ci, vals = oracle.assemble(asm)
        K = sp.csr_matrix((vals, ci.astype(np.int64), ro.astype(np.int64)), shape=(len(u), len(u))).toarray()
        q = np.zeros_like(u)
        q[free] = np.linalg.solve(K[np.ix_(free, free)], F[free])
        step = -q
        if not backtracking:
            u = u + step
            F, asm = residual(u)
            evals += 1
            steps.append(1.0)
        else:
            g0, a_prev, a = 0.5 * fn * fn, 0.0, 1.0
            while True:
                u = u + (a - a_prev) * step
                F, asm = residual(u)
                evals += 1
                if 0.5 * np.dot(F, F) <= (1.0 - 1e-4 * a) * g0:
                    break
                if a < 1e-6:
                    return "line_search", u, it, evals, steps
                a_prev, a = a, {1.0: 0.75, 0.75: 0.5, 0.5: 0.25}.get(a, 0.25 * a)
            steps.append(a)
        it += 1


def _det_f(m, w, p, u, kind):
    """det F = det(I + grad u) at every quadrature point (NumPy, on the geometry of the linear kinds)"""
    from oracle import oracle as o

    d = m.vertices.shape[1]
    G = [o.element_gradients(OKIND[kind], xi) for xi in p]
    out = []
    for e in m.connectivity.astype(np.int64):
        X, U = m.vertices[e], u.reshape(-1, d)[e]
        for g in G:
            J = X.T @ g.T
            out.append(np.linalg.det(np.eye(d) + U.T @ g.T @ np.linalg.inv(J)))
    return np.array(out)


def _accepted_steps(asm, clamp, f, tol, iterations, u0=None):
    """the accepted step length of every iteration: solves from the same guess stopped after k = 1 .. iterations (their last steps)"""
    steps = []
    for k in range(1, iterations + 1):
        u = np.zeros_like(f) if u0 is None else u0.copy()
        try:
            res = fa.MatrixFreeNewton(asm).with_dirichlet_nodes(clamp).with_load(f).solve(u, fa.NewtonSettings(k, tol), linear_rel_tol=1e-12)
        except fa.MaximumIterationsReached as e:
            res = e.result
        steps.append(res.step_length)
    return steps


def test_newton_entry_points_are_declared():
    """no GPU: the header, the bindings and the package know the solver"""
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fenris_hip.h")).read()
    for name in ("fh_newton_solve", "fh_newton_solve_dev"):
        assert name in _ffi.exported_symbols() and name + "(" in hdr
    for name in ("FH_NEWTON_MAX_ITERATIONS = 10", "FH_NEWTON_JACOBIAN_ERROR = 11", "FH_NEWTON_LINE_SEARCH_FAILED = 12", "FH_NEWTON_BACKTRACKING = 1"):
        assert name in hdr
    assert issubclass(fa.MaximumIterationsReached, fa.NewtonError) and issubclass(fa.JacobianError, fa.NewtonError)
    assert issubclass(fa.LineSearchError, fa.NewtonError) and fa.NewtonSettings().max_iterations is None


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["HEX8", "TET4", "QUAD4", "TET10"])
@pytest.mark.parametrize("op", ["neo_hookean", "stvk"])
def test_cpu_parity(engine, oracle, kind, op):
    m, w, p = _mesh(kind)
    clamp, f = _clamped_pull(m, 2e5)
    tol = 1e-8 * np.linalg.norm(f)
    ref = _np_newton(oracle, kind, op, m, w, p, np.zeros_like(f), f, clamp, tol)
    assert ref[0] == "ok"
    asm = _assembler(engine, m, w, p, op)
    u = np.zeros_like(f)
    res = fa.MatrixFreeNewton(asm).with_dirichlet_nodes(clamp).with_load(f).solve(u, fa.NewtonSettings(60, tol), linear_rel_tol=1e-12)
    assert (res.iterations, res.residual_evaluations) == (ref[2], ref[3])
    assert _accepted_steps(asm, clamp, f, tol, res.iterations) == ref[4]
    assert res.residual_norm <= tol and res.linear_status == 0
    assert np.abs(u - ref[1]).max() <= 1e-8 * np.abs(ref[1]).max()


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["laplace", "elastic"])
@pytest.mark.parametrize("kind", ["HEX8", "TET4"])
def test_linear_operator_converges_in_one_iteration(engine, kind, op):
    """newton_converges_in_single_iteration_for_linear_system, and the solution is the matrix-free CG's"""
    m, w, p = _mesh(kind)
    s = 1 if op == "laplace" else 3
    clamp, f = _clamped_pull(m, 1e3, s)
    f += 10.0 * np.sin(np.arange(len(f)))
    f_free = f.copy()
    for k in range(s):
        f_free[s * clamp + k] = 0.0
    asm = _assembler(engine, m, w, p, op)
    tol = 1e-8 * np.linalg.norm(f_free)
    u = np.zeros_like(f)
    res = fa.MatrixFreeNewton(asm).with_dirichlet_nodes(clamp).with_load(f).solve(u, fa.NewtonSettings(None, tol), linear_rel_tol=1e-12)
    assert res.iterations == 1 and res.residual_evaluations == 2 and res.step_length == 1.0
    x = np.zeros_like(f)
    asm.with_u(np.zeros_like(f))
    fa.MatrixFreeOperator(asm).with_dirichlet_nodes(clamp).cg_solve(f_free, x, 1, 1e-12)
    assert np.abs(u - x).max() <= 1e-9 * np.abs(x).max()


@pytest.mark.gpu
def test_backtracking_passes_inverted_trials_and_the_full_step_fails(engine, oracle):
    """NeoHookean block clamped on x = 0 and pulled hard on x = 1: the full first step inverts elements (NaN residual).  Backtracking passes
    over the NaN trials, accepts steps below 1 and converges with every det F > 0, as the NumPy Newton does; the full step is a failure."""
    m, w, p = _mesh("HEX8")
    clamp, f = _clamped_pull(m, 2.5e6)
    tol = 1e-8 * np.linalg.norm(f)
    ref = _np_newton(oracle, "HEX8", "neo_hookean", m, w, p, np.zeros_like(f), f, clamp, tol)
    full = _np_newton(oracle, "HEX8", "neo_hookean", m, w, p, np.zeros_like(f), f, clamp, tol, backtracking=False, max_it=1)
    assert ref[0] == "ok" and min(ref[4]) < 1.0 and full[0] == "nonfinite"
    asm = _assembler(engine, m, w, p, "neo_hookean")
    solver = fa.MatrixFreeNewton(asm).with_dirichlet_nodes(clamp).with_load(f)
    u = np.zeros_like(f)
    res = solver.solve(u, fa.NewtonSettings(60, tol), linear_rel_tol=1e-12)
    assert res.residual_norm <= tol and res.linear_status == 0
    assert (res.iterations, res.residual_evaluations) == (ref[2], ref[3])
    assert _accepted_steps(asm, clamp, f, tol, res.iterations) == ref[4]
    assert (_det_f(m, w, p, u, "HEX8") > 0).all()
    assert np.abs(u - ref[1]).max() <= 1e-8 * np.abs(ref[1]).max()
    # the full step reaches a NaN residual: a failure, not a success (newton.rs would report success here)
    u2 = np.zeros_like(f)
    with pytest.raises(fa.LineSearchError) as ei:
        solver.solve(u2, fa.NewtonSettings(60, tol), line_search=fa.NoLineSearch(), linear_rel_tol=1e-12)
    assert ei.value.code == _ffi.FH_NEWTON_LINE_SEARCH_FAILED
    assert ei.value.result.iterations == 1 and np.isnan(ei.value.result.residual_norm) and np.isfinite(u2).all()
    assert not (_det_f(m, w, p, u2, "HEX8") > 0).all()
    assert np.abs(u2 - full[1]).max() <= 1e-8 * np.abs(full[1]).max()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["HEX8", "TET10"])
def test_inhomogeneous_dirichlet_values_are_kept_bitwise(engine, oracle, kind):
    m, w, p = _mesh(kind)
    x = m.vertices
    clamp = np.where(np.isclose(x[:, 0], 0.0))[0]
    pulled = np.where(np.isclose(x[:, 0], 1.0))[0]
    nodes = np.concatenate([clamp, pulled])
    u0 = np.zeros(3 * len(x))
    u0[3 * pulled] = 0.3
    u0[3 * pulled + 1] = 0.05 * x[pulled, 2]
    f = np.zeros_like(u0)
    ref = _np_newton(oracle, kind, "neo_hookean", m, w, p, u0, f, nodes, 1e-6)
    assert ref[0] == "ok"
    asm = _assembler(engine, m, w, p, "neo_hookean")
    u = u0.copy()
    res = fa.MatrixFreeNewton(asm).with_dirichlet_nodes(nodes).solve(u, fa.NewtonSettings(60, 1e-6), linear_rel_tol=1e-12)
    assert res.iterations == ref[2] and res.residual_norm <= 1e-6
    fixed = np.zeros(len(u), dtype=bool)
    for k in range(3):
        fixed[3 * nodes + k] = True
    assert np.array_equal(u[fixed].view(np.uint64), u0[fixed].view(np.uint64))
    assert np.abs(u - ref[1]).max() <= 1e-8 * np.abs(ref[1]).max()


def _mass_csr(m, w, p, rho, s):
    meng = fa.Engine(0)
    qt = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(fa.Density(rho))
    masm = fa.ElementMassAssembler.with_solution_dim(s, meng).with_space(m).with_quadrature_table(qt)
    return fa.CsrAssembler(fa.SCATTER_GATHER).assemble(masm).to_scipy()


def _implicit_problem(m):
    x = m.vertices
    clamp, f = _clamped_pull(m, 1e3)
    u_ref = np.zeros_like(f)
    u_ref[0::3] = 0.02 * x[:, 0] ** 2
    u_ref[1::3] = 0.01 * np.sin(np.pi * x[:, 0])
    for k in range(3):
        u_ref[3 * clamp + k] = 0.0
    return clamp, f, u_ref


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["HEX8", "TET4", "TET10"])
def test_implicit_step_satisfies_the_assembled_equations(engine, kind):
    import torch

    m, w, p = _mesh(kind)
    rho, dt = 1e3, 1e-2
    clamp, f, u_ref = _implicit_problem(m)
    asm = _assembler(engine, m, w, p, "neo_hookean")
    tol = 1e-9
    u = torch.tensor(u_ref, device="cuda:0")
    res = (fa.MatrixFreeNewton(asm).with_dirichlet_nodes(clamp).with_load(torch.tensor(f, device="cuda:0"))
           .with_inertia(rho, 1.0, dt * dt, torch.tensor(u_ref, device="cuda:0")).solve(u, fa.NewtonSettings(30, tol)))
    assert res.iterations >= 1 and res.residual_norm <= tol
    uh = u.cpu().numpy()
    M = _mass_csr(m, w, p, rho, 3)
    asm.with_u(uh)
    r = fa.VectorAssembler().assemble_vector(asm)
    F = M @ (uh - u_ref) + dt * dt * (r - f)
    for k in range(3):
        F[3 * clamp + k] = 0.0
    assert np.linalg.norm(F) <= tol * (1 + 1e-6) + 1e-14 * (np.abs(M @ (uh - u_ref)).max() + dt * dt * np.abs(r).max()) * np.sqrt(len(F))


def _composed_norm(engine, asm, m, clamp, rho, alpha, beta, u0, u_ref, f):
    """||alpha M (u0 - u_ref) + beta (r(u0) - f)|| with the Dirichlet rows zero, from the existing entry points"""
    import torch

    asm.with_u(u0)
    r = fa.VectorAssembler().assemble_vector(asm)
    sh = fa.MatrixFreeShiftedTangent(asm, rho, 1.0, 0.0)   # (alpha = 1, beta = 0: M x)
    md = np.zeros_like(u0)
    sh.apply(md, u0 - u_ref)
    F = alpha * md + beta * (r - f)
    for k in range(3):
        F[3 * clamp + k] = 0.0
    return np.linalg.norm(F)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["HEX8", "TET4"])
@pytest.mark.parametrize("table", ["uniform", "rule_set"])
def test_fused_residual_and_norm(engine, kind, table):
    m, w, p = _mesh(kind)
    rho, alpha, beta = 2e3, 1.0, 1e-3
    clamp, f, u_ref = _implicit_problem(m)
    u0 = 0.5 * u_ref + 0.003 * np.cos(np.arange(len(f)))
    for k in range(3):
        u0[3 * clamp + k] = 0.0
    qt = None
    if table == "rule_set":
        w2, p2 = (np.asarray(a) for a in (quadrature.tensor.hexahedron_gauss(3) if kind == "HEX8" else quadrature.total_order.tetrahedron(4)))
        emap = (np.arange(m.num_elements()) % 2).astype(np.uint64)
        qt = fa.compact_quadrature_table([p, p2], [w, w2], [[LAME] * len(w), [LAME] * len(w2)], emap)
    asm = _assembler(engine, m, w, p, "neo_hookean", qt=qt)
    solver = fa.MatrixFreeNewton(asm).with_dirichlet_nodes(clamp).with_load(f).with_inertia(rho, alpha, beta, u_ref)
    u = u0.copy()
    res = solver.solve(u, fa.NewtonSettings(None, 1e300))   # converged on entry: one evaluation of F and its norm
    assert res.iterations == 0 and res.residual_evaluations == 1 and np.array_equal(u, u0)
    route = engine.last_kernel_name()
    assert ("k_newton_from_partials" in route) == (table == "uniform"), route
    assert ("k_mass_tiled" in route) == (table == "uniform"), route
    assert route == ("k_element_pass_tiled + k_mass_tiled + k_newton_from_partials" if table == "uniform"
                     else "k_residual_elements + k_vector_from_elements_soa + k_newton_combine"), route
    ref = _composed_norm(engine, asm, m, clamp, rho, alpha, beta, u0, u_ref, f)
    assert abs(res.initial_residual_norm - ref) <= 1e-13 * ref
    # the static residual (alpha = 0: no mass partials) takes the same two routes; its norm against the same composition
    static = fa.MatrixFreeNewton(asm).with_dirichlet_nodes(clamp).with_load(f)
    res0 = static.solve(u0.copy(), fa.NewtonSettings(None, 1e300))
    route0 = engine.last_kernel_name()
    assert route0 == ("k_element_pass_tiled + k_newton_from_partials" if table == "uniform"
                      else "k_residual_elements + k_vector_from_elements_soa + k_newton_combine"), route0
    ref0 = _composed_norm(engine, asm, m, clamp, rho, 0.0, 1.0, u0, u_ref, f)
    assert abs(res0.initial_residual_norm - ref0) <= 1e-13 * ref0
    # F itself: one Newton step from u0 through the fused pass against the same step with the tiles switched off (the composed route)
    u1 = u0.copy()
    with pytest.raises(fa.MaximumIterationsReached):
        solver.solve(u1, fa.NewtonSettings(1, 1e-30), line_search=fa.NoLineSearch(), linear_rel_tol=1e-12)
    os.environ["FENRIS_HIP_NO_VECTOR_TILES"] = "1"
    try:
        eng2 = fa.Engine(0)
    finally:
        del os.environ["FENRIS_HIP_NO_VECTOR_TILES"]
    asm2 = _assembler(eng2, m, w, p, "neo_hookean", qt=qt)
    u2 = u0.copy()
    with pytest.raises(fa.MaximumIterationsReached) as ei:
        (fa.MatrixFreeNewton(asm2).with_dirichlet_nodes(clamp).with_load(f).with_inertia(rho, alpha, beta, u_ref)
         .solve(u2, fa.NewtonSettings(1, 1e-30), line_search=fa.NoLineSearch(), linear_rel_tol=1e-12))
    assert "k_newton_combine" in eng2.last_kernel_name()
    assert abs(ei.value.result.initial_residual_norm - ref) <= 1e-13 * ref
    assert np.abs(u1 - u2).max() <= 1e-9 * np.abs(u1 - u0).max()
    eng2.close()


@pytest.mark.gpu
def test_contract(engine):
    import torch

    m, w, p = _mesh("HEX8")
    clamp, f = _clamped_pull(m, 2e5)
    asm = _assembler(engine, m, w, p, "neo_hookean")
    solver = fa.MatrixFreeNewton(asm).with_dirichlet_nodes(clamp).with_load(f)
    tol = 1e-8 * np.linalg.norm(f)
    # two solves repeat bitwise (device tensors)
    outs = []
    for _ in range(2):
        u = torch.zeros(len(f), dtype=torch.float64, device="cuda:0")
        res = solver.solve(u, fa.NewtonSettings(60, tol))
        outs.append((u.cpu().numpy(), res))
    assert np.array_equal(outs[0][0].view(np.uint64), outs[1][0].view(np.uint64)) and outs[0][1] == outs[1][1]
    # max_iterations: u is the last iterate
    u = np.zeros_like(f)
    with pytest.raises(fa.MaximumIterationsReached) as ei:
        solver.solve(u, fa.NewtonSettings(2, tol))
    assert ei.value.code == _ffi.FH_NEWTON_MAX_ITERATIONS and ei.value.iterations == 2 and ei.value.result.iterations == 2
    u3 = np.zeros_like(f)
    with pytest.raises(fa.MaximumIterationsReached):
        solver.solve(u3, fa.NewtonSettings(3, tol))
    u_again = u.copy()   # (one more iteration from the 2nd iterate: the 3rd)
    with pytest.raises(fa.MaximumIterationsReached):
        solver.solve(u_again, fa.NewtonSettings(1, tol))
    assert np.abs(u_again - u3).max() <= 1e-10 * np.abs(u3).max()
    # an already converged guess: 0 iterations, 1 evaluation, u untouched
    uc = outs[0][0].copy()
    res = solver.solve(uc, fa.NewtonSettings(60, tol))
    assert res.iterations == 0 and res.residual_evaluations == 1 and res.step_length == 0.0
    assert np.array_equal(uc, outs[0][0])
    # the engine's u is the solution afterwards
    r = fa.VectorAssembler().assemble_vector(asm) - f
    r[np.repeat(clamp * 3, 3) + np.tile(np.arange(3), len(clamp))] = 0.0
    assert np.linalg.norm(r) <= tol
    # Jacobian error: the inner PCG hits its iteration limit
    with pytest.raises(fa.JacobianError) as ej:
        solver.solve(np.zeros_like(f), fa.NewtonSettings(60, tol), linear_max_iter=2)
    assert ej.value.code == _ffi.FH_NEWTON_JACOBIAN_ERROR and ej.value.cg_code == 7
    # arguments and state
    lib, h = engine._lib, engine._h
    st = np.zeros(4, dtype=np.uint64)
    nm = np.zeros(3)
    ub = np.zeros_like(f)
    call = lambda a, b, tol_, u_: lib.fh_newton_solve(h, a, b, None, None, _ffi.fp(u_) if u_ is not None else None, tol_, 0, 1, 1, 1e-8, 0,
                                                     _ffi.up(st), _ffi.fp(nm))
    assert call(0.0, 1.0, float("nan"), ub) == FH_BAD_ARGUMENT
    assert call(0.0, 1.0, 1e-6, None) == FH_BAD_ARGUMENT
    assert call(float("inf"), 1.0, 1e-6, ub) == FH_BAD_ARGUMENT
    assert call(1.0, 1.0, 1e-6, ub) == FH_INVALID_STATE   # no density
    for kind in (_ffi.MASS_VECTOR, _ffi.TENSOR):
        e2 = fa.Engine(0)
        e2.set_mesh(m)
        e2.set_operator(kind)
        ub2 = np.zeros_like(f)
        assert e2._lib.fh_newton_solve(e2._h, 0.0, 1.0, None, None, _ffi.fp(ub2), 1e-6, 0, 1, 1, 1e-8, 0, None, None) == FH_UNSUPPORTED
        e2.close()


def _fma_exact(a, b, c):
    """round(a b + c) once, as the device's fma (through exact rationals)"""
    from fractions import Fraction

    return np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(np.broadcast_to(a, np.shape(c)), b, c)])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,implicit", [("HEX8", False), ("TET4", False), ("TET4", True), ("QUAD4", False)])
def test_fused_residual_elementwise(engine, kind, implicit):
    """F of the fused node pass equals alpha M d + beta (r - f) from the existing entry points bit for bit: the step of one Newton iteration
    is the existing shifted PCG (fh_cg_solve_shifted_tangent_dev) run on that reference F, and the PCG is deterministic, so any bit of F that
    differed would show in u."""
    import torch

    m, w, p = _mesh(kind)
    s = m.vertices.shape[1]
    rho, alpha, beta = (2e3, 1.0, 1e-3) if implicit else (None, 0.0, 1.0)
    x = m.vertices
    clamp, f = _clamped_pull(m, 1e4)
    u_ref = np.zeros_like(f)
    u_ref[0::s] = 0.01 * x[:, 0] ** 2
    u0 = 0.5 * u_ref + 0.003 * np.cos(np.arange(len(f)))
    for k in range(s):
        u0[s * clamp + k] = 0.0
    asm = _assembler(engine, m, w, p, "neo_hookean")
    # the reference F from the existing entry points: r(u0) (tile residual), M d (the shifted map with beta = 0, no Dirichlet nodes)
    asm.with_u(u0)
    r = fa.VectorAssembler().assemble_vector(asm)
    F = (r - f) if beta == 1.0 and alpha == 0.0 else None
    if implicit:
        md = np.zeros_like(f)
        fa.MatrixFreeShiftedTangent(asm, rho, 1.0, 0.0).apply(md, u0 - u_ref)
        F = _fma_exact(beta, r - f, alpha * md)
    for k in range(s):
        F[s * clamp + k] = 0.0
    # the step the existing PCG takes on it (Dirichlet nodes bound, u = u0, zero guess)
    sh = fa.MatrixFreeShiftedTangent(asm, rho if implicit else 1.0, alpha, beta).with_dirichlet_nodes(clamp)
    asm.with_u(u0)
    q = torch.zeros(len(f), dtype=torch.float64, device="cuda:0")
    sh.cg_solve(torch.tensor(F, device="cuda:0"), q, 1, 1e-12, 0)
    expect = u0 - q.cpu().numpy()
    solver = fa.MatrixFreeNewton(asm).with_dirichlet_nodes(clamp).with_load(f)
    if implicit:
        solver.with_inertia(rho, alpha, beta, u_ref)
    u = u0.copy()
    with pytest.raises(fa.MaximumIterationsReached) as ei:
        solver.solve(u, fa.NewtonSettings(1, 0.0), line_search=fa.NoLineSearch(), linear_rel_tol=1e-12)
    assert abs(ei.value.result.initial_residual_norm - np.linalg.norm(F)) <= 1e-13 * np.linalg.norm(F)
    assert np.array_equal(u.view(np.uint64), expect.view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["TET10", "HEX8"])
def test_off_tile_route_repeats_bitwise(engine, kind):
    """Tet10 takes the composed route (k_residual_elements, ordered node sums, no atomics), a rule-set table on Hex8 as well: two solves
    repeat bit for bit"""
    m, w, p = _mesh(kind)
    clamp, f = _clamped_pull(m, 2e5)
    qt = None
    if kind == "HEX8":
        w2, p2 = (np.asarray(a) for a in quadrature.tensor.hexahedron_gauss(3))
        emap = (np.arange(m.num_elements()) % 2).astype(np.uint64)
        qt = fa.compact_quadrature_table([p, p2], [w, w2], [[LAME] * len(w), [LAME] * len(w2)], emap)
    asm = _assembler(engine, m, w, p, "neo_hookean", qt=qt)
    solver = fa.MatrixFreeNewton(asm).with_dirichlet_nodes(clamp).with_load(f).with_inertia(1e3, 1.0, 1e-4, 0.01 * np.sin(np.arange(len(f))))
    outs = []
    for _ in range(2):
        u = np.zeros_like(f)
        res = solver.solve(u, fa.NewtonSettings(30, 1e-8 * np.linalg.norm(f)))
        outs.append((u, res))
        assert "k_residual_elements" in engine.last_kernel_name()
    assert outs[0][1].iterations >= 1 and outs[0][1] == outs[1][1]
    assert np.array_equal(outs[0][0].view(np.uint64), outs[1][0].view(np.uint64))


@pytest.mark.gpu
def test_solve_checks_its_vectors(engine):
    import torch

    m, w, p = _mesh("HEX8")
    clamp, f = _clamped_pull(m, 1e3)
    solver = fa.MatrixFreeNewton(_assembler(engine, m, w, p, "neo_hookean")).with_dirichlet_nodes(clamp).with_load(f)
    for bad in (torch.zeros(len(f), dtype=torch.float32, device="cuda:0"), torch.zeros(len(f) - 3, dtype=torch.float64, device="cuda:0"),
                torch.zeros(2 * len(f), dtype=torch.float64, device="cuda:0")[::2], np.zeros(len(f) - 1)):
        with pytest.raises(ValueError):
            solver.solve(bad)
    with pytest.raises(ValueError):
        fa.MatrixFreeNewton(solver.element_assembler).with_load(f[:-1]).solve(np.zeros_like(f))
