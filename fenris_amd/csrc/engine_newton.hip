// Newton's method on the device (fenris-optimize/src/newton.rs): the loop of newton_line_search around the Newton residual of
// engine_vector.hip and the matrix-free shifted PCG of engine_solver.hip; C ABI
#include "engine_internal.hpp"

#include <cmath>

namespace {

// BacktrackingLineSearch's trial step lengths after `a` (newton.rs:212-218): 1, 0.75, 0.5, then 0.25, 0.0625, ... (0.25 each time)
double next_step_length(double a) {
    if (a == 1.0) return 0.75;
    if (a == 0.75) return 0.5;
    if (a == 0.5) return 0.25;
    return 0.25 * a;
}

}  // namespace

// newton_line_search (newton.rs:77-130) for F(u) = alpha M (u - u_ref) + beta (r(u) - f).  The iterate is the context's u, moved in place
// (k_newton_move, which also forms d = u - u_ref for the mass term), so that every residual evaluation reads it where it lies; u_gen moves with
// every move.  Each Newton step solves J q = F (q = -dx of newton.rs:109-117) by the matrix-free shifted PCG from a zero guess; the step is p = -q.
int newton_run(fh_ctx* c, double alpha, double beta, const double* f, const double* u_ref, double tolerance, uint64_t max_iterations,
                      int line_search, int preconditioner, double linear_rel_tol, uint64_t linear_max_iter, uint64_t* st, double* nm) {
    const char* who = "fh_newton_solve";
    if (preconditioner == FH_PRECOND_MULTIGRID && contact_table(c).count)
        return c->fail(FH_UNSUPPORTED, std::string(who) + ": FH_PRECOND_MULTIGRID with obstacles set (fh_set_obstacles): the coarse levels would not see the contact term");
    if (preconditioner == FH_PRECOND_MULTIGRID) {   // (nor the per-element expansion of a hyperelastic operator)
        const int rb = expansion_blocks_multigrid(c, who);
        if (rb) return rb;
    }
    const int n = c->S() * (int)c->N;
    const int g = (n + 255) / 256;
    NewtonScratch ns;
    DevBuf<double> q, d;   // (allocated once per solve)
    HIP_TRY(c, q.alloc((size_t)n));
    if (alpha != 0.0) HIP_TRY(c, d.alloc((size_t)n));
    auto move = [&](double da, const double* step) -> int {
        hipLaunchKernelGGL(k_newton_move, dim3(g), dim3(256), 0, c->stream, n, da, step, c->u.p, u_ref, alpha != 0.0 ? d.p : nullptr);
        HIP_TRY(c, hipGetLastError());
        if (step) ++c->u_gen;
        return (int)FH_OK;
    };
    auto eval = [&](double* norm) -> int {
        double norm2 = 0.0;
        const int rc = newton_residual(c, alpha, beta, f, d.p, ns, &norm2);
        if (rc) return rc;
        ++st[1];
        *norm = std::sqrt(norm2);
        return (int)FH_OK;
    };
    int rc = alpha != 0.0 ? move(0.0, nullptr) : FH_OK;   // d = u_0 - u_ref
    if (rc) return rc;
    double fnorm;
    rc = eval(&fnorm);
    if (rc) return rc;
    nm[0] = nm[1] = fnorm;
    for (;;) {
        // (newton.rs:98 exits on a NaN norm and reports success; here a non-finite norm of an accepted state ends the solve as a failure)
        if (!std::isfinite(fnorm)) return c->fail(FH_NEWTON_LINE_SEARCH_FAILED, std::string(who) + ": the residual norm is not finite");
        if (fnorm <= tolerance) return FH_OK;
        if (max_iterations && st[0] == max_iterations)
            return c->fail(FH_NEWTON_MAX_ITERATIONS, std::string(who) + ": failed to converge within the maximum number of iterations");
        HIP_TRY(c, hipMemsetAsync(q.p, 0, sizeof(double) * (size_t)n, c->stream));
        uint64_t cg_it = 0;
        const int rcg = cg_solve_free_dev(c, who, MF_TANGENT, ns.F.p, q.p, preconditioner, linear_rel_tol, linear_max_iter, &cg_it, alpha, beta);
        st[2] += cg_it;
        st[3] = (uint64_t)rcg;
        // (any error of solve_jacobian_system is a JacobianError, newton.rs:112-115: the PCG's own codes and what its map reports, e.g.
        // FH_SINGULAR_JACOBIAN; stats[3] keeps the code, the message its text)
        if (rcg) return c->fail(FH_NEWTON_JACOBIAN_ERROR, std::string(who) + ": failed to solve the Jacobian system: " + c->err);
        if (line_search == FH_NEWTON_NO_LINE_SEARCH) {   // NoLineSearch (newton.rs:151-163)
            rc = move(1.0, q.p);
            if (rc) return rc;
            rc = eval(&fnorm);
            if (rc) return rc;
            nm[1] = fnorm;
            nm[2] = 1.0;
        } else {   // BacktrackingLineSearch (newton.rs:172-249): g = |F|^2 / 2, accept g <= (1 - c a) g_0, fail below a = 1e-6
            const double c_armijo = 1e-4, a_min = 1e-6;
            const double g0 = 0.5 * fnorm * fnorm;
            double a_prev = 0.0, a = 1.0;
            for (;;) {
                rc = move(a - a_prev, q.p);   // x^{k+1} = x^k + (a^k - a^{k-1}) p
                if (rc) return rc;
                rc = eval(&fnorm);
                if (rc) return rc;
                nm[1] = fnorm;
                const double gv = 0.5 * fnorm * fnorm;
                if (gv <= (1.0 - c_armijo * a) * g0) break;   // (a NaN residual compares false: the search backtracks past it)
                if (a < a_min)
                    return c->fail(FH_NEWTON_LINE_SEARCH_FAILED, std::string(who) + ": the line search found no step length above 1e-6");
                a_prev = a;
                a = next_step_length(a);
            }
            nm[2] = a;
        }
        ++st[0];
    }
}

static int newton_solve_dev(fh_ctx* c, double alpha, double beta, const double* f_dev, const double* u_ref_dev, double* u_dev, double tolerance,
                            uint64_t max_iterations, int line_search, int preconditioner, double linear_rel_tol, uint64_t linear_max_iter,
                            uint64_t* stats, double* norms) {
    const char* who = "fh_newton_solve";
    uint64_t st[4] = {0, 0, 0, 0};
    double nm[3] = {0.0, 0.0, 0.0};
    if (stats) std::copy(st, st + 4, stats);
    if (norms) std::copy(nm, nm + 3, norms);
    int rc = mf_shift_ready(c, who, alpha, beta);
    if (rc) return rc;
    if (!std::isfinite(tolerance)) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": the tolerance must be finite");
    if (!u_dev) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": u is null");
    if (line_search != FH_NEWTON_NO_LINE_SEARCH && line_search != FH_NEWTON_BACKTRACKING)
        return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": unknown line search");
    if (preconditioner != FH_PRECOND_IDENTITY && preconditioner != FH_PRECOND_JACOBI && preconditioner != FH_PRECOND_MULTIGRID)
        return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": unknown preconditioner");
    if (c->N == 0) return FH_OK;
    rc = fh_set_u_dev(c, u_dev);   // the iterate lives in the context's u
    if (rc) return rc;
    rc = newton_run(c, alpha, beta, f_dev, u_ref_dev, tolerance, max_iterations, line_search, preconditioner, linear_rel_tol, linear_max_iter, st, nm);
    if (stats) std::copy(st, st + 4, stats);
    if (norms) std::copy(nm, nm + 3, norms);
    // u as the reference leaves x, on success and on failure
    HIP_TRY(c, hipMemcpyAsync(u_dev, c->u.p, sizeof(double) * (size_t)c->S() * c->N, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return rc;
}

extern "C" {

int fh_newton_solve_dev(fh_ctx* c, double alpha, double beta, const double* f_dev, const double* u_ref_dev, double* u_dev, double tolerance,
                        uint64_t max_iterations, int line_search, int preconditioner, double linear_rel_tol, uint64_t linear_max_iter,
                        uint64_t* stats, double* norms) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    return newton_solve_dev(c, alpha, beta, f_dev, u_ref_dev, u_dev, tolerance, max_iterations, line_search, preconditioner, linear_rel_tol,
                            linear_max_iter, stats, norms);
}

int fh_newton_solve(fh_ctx* c, double alpha, double beta, const double* f, const double* u_ref, double* u, double tolerance, uint64_t max_iterations,
                    int line_search, int preconditioner, double linear_rel_tol, uint64_t linear_max_iter, uint64_t* stats, double* norms) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (stats) std::fill(stats, stats + 4, 0);
    if (norms) std::fill(norms, norms + 3, 0.0);
    int rc = mf_shift_ready(c, "fh_newton_solve", alpha, beta);
    if (rc) return rc;
    if (!u) return c->fail(FH_BAD_ARGUMENT, "fh_newton_solve: u is null");
    const size_t n = (size_t)c->S() * c->N;
    DevBuf<double> df, dr, du;
    HIP_TRY(c, du.alloc(n + 1));
    HIP_TRY(c, hipMemcpyAsync(du.p, u, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    if (f) {
        HIP_TRY(c, df.alloc(n + 1));
        HIP_TRY(c, hipMemcpyAsync(df.p, f, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    }
    if (u_ref) {
        HIP_TRY(c, dr.alloc(n + 1));
        HIP_TRY(c, hipMemcpyAsync(dr.p, u_ref, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    }
    rc = newton_solve_dev(c, alpha, beta, f ? df.p : nullptr, u_ref ? dr.p : nullptr, du.p, tolerance, max_iterations, line_search, preconditioner,
                          linear_rel_tol, linear_max_iter, stats, norms);
    HIP_TRY(c, hipMemcpyAsync(u, du.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return rc;
}

}  // extern "C"
