// Dirichlet rows, SpMV, Jacobi-PCG, error integrals: C ABI
#include <functional>

#include "engine_internal.hpp"

// (dm_dev null: the checks alone)
extern "C++" int dirichlet_masks_to_device(fh_ctx* c, const char* who, const uint64_t* nodes, const uint8_t* components, uint64_t num_nodes,
                                           unsigned char* dm_dev, uint64_t (&comp_node)[8]) {
    std::fill(comp_node, comp_node + 8, (uint64_t)0);
    for (uint64_t i = 0; i < num_nodes; ++i) {
        if (nodes[i] >= c->N) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": Dirichlet node " + std::to_string(nodes[i]) + " out of range");
        if (!components) continue;
        const unsigned m = components[i];
        if (m == 0) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": node " + std::to_string(nodes[i]) + " has a component mask of 0");
        if (m == DMASK_NODE) continue;
        for (int j = 0; j < 8; ++j)
            if (((m >> j) & 1u) && !comp_node[j]) comp_node[j] = nodes[i] + 1;
    }
    if (!dm_dev || !num_nodes) return FH_OK;
    DevBuf<unsigned long long> dn;
    DevBuf<unsigned char> dc;
    HIP_TRY(c, dn.alloc((size_t)num_nodes));
    HIP_TRY(c, hipMemcpyAsync(dn.p, nodes, sizeof(uint64_t) * num_nodes, hipMemcpyHostToDevice, c->stream));
    if (components) {
        HIP_TRY(c, dc.alloc((size_t)num_nodes));
        HIP_TRY(c, hipMemcpyAsync(dc.p, components, (size_t)num_nodes, hipMemcpyHostToDevice, c->stream));
    }
    hipLaunchKernelGGL(k_mark_dofs, dim3(grid_for((long long)num_nodes, 256, 1 << 30)), dim3(256), 0, c->stream, dn.p,
                       components ? (const unsigned char*)dc.p : nullptr, (long long)num_nodes, dm_dev);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // (dn and dc are released on return)
    return FH_OK;
}

extern "C++" int dirichlet_components_fit(fh_ctx* c, const char* who, const uint64_t (&comp_node)[8], int S) {
    for (int j = S < 0 ? 0 : S; j < 8; ++j)
        if (comp_node[j])
            return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": Dirichlet node " + std::to_string(comp_node[j] - 1) + " constrains component " +
                                                std::to_string(j) + ", the operator's solution has " + std::to_string(S));
    return FH_OK;
}

extern "C" {
int fh_apply_dirichlet_csr_dev(fh_ctx* c, double* values_dev, const uint64_t* nodes, uint64_t n) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (!c->has_pattern) return c->fail(FH_INVALID_STATE, "fh_apply_dirichlet_csr_dev: call fh_pattern first");
    if (!values_dev || (n && !nodes)) return c->fail(FH_BAD_ARGUMENT, "fh_apply_dirichlet_csr_dev: null pointer");
    const int S = c->S(), N = (int)c->N;
    for (uint64_t i = 0; i < n; ++i)
        if (nodes[i] >= c->N) return c->fail(FH_BAD_ARGUMENT, "Dirichlet node out of range");
    // membership flags on the device from the node list (round 4: a host array of N bytes filled and uploaded per call, an entry-wise
    // kernel that searched each entry's row by bisection and a host round trip for the scale made this step 11 ms on the 216^3 mesh)
    DevBuf<unsigned char> dm;
    DevBuf<unsigned long long> first, dn;
    DevBuf<double> scale;
    HIP_TRY(c, dm.alloc((size_t)N + 1));
    HIP_TRY(c, first.alloc(1));
    HIP_TRY(c, scale.alloc(1));
    HIP_TRY(c, dn.alloc((size_t)n + 1));
    HIP_TRY(c, hipMemsetAsync(dm.p, 0, (size_t)N + 1, c->stream));
    if (n) {
        HIP_TRY(c, hipMemcpyAsync(dn.p, nodes, sizeof(uint64_t) * n, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_mark_nodes, dim3(grid_for((long long)n, 256, 1 << 30)), dim3(256), 0, c->stream, dn.p, (long long)n, dm.p);
    }
    HIP_TRY(c, hipMemsetAsync(first.p, 0xff, sizeof(unsigned long long), c->stream));
    const long long R = (long long)N * S;
    hipLaunchKernelGGL(k_first_nonzero_diag, dim3(grid_for(R, 256, 1 << 30)), dim3(256), 0, c->stream, c->noff.p, c->ncols.p, N, S,
                       values_dev, first.p, (double*)nullptr);
    hipLaunchKernelGGL(k_first_nonzero_diag, dim3(1), dim3(64), 0, c->stream, c->noff.p, c->ncols.p, N, S, values_dev, first.p,
                       scale.p);
    if (c->nnz_nodes)
        hipLaunchKernelGGL(k_dirichlet_rows, dim3(grid_for(((long long)N + 7) / 8, 1, 1 << 20)), dim3(256), 0, c->stream, c->noff.p,
                           c->ncols.p, N, S, dm.p, values_dev, scale.p);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the temporaries are released on return)
    return FH_OK;
}

int fh_apply_dirichlet_dofs_csr_dev(fh_ctx* c, double* values_dev, const uint64_t* nodes, const uint8_t* components, uint64_t n) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (!c->has_pattern) return c->fail(FH_INVALID_STATE, "fh_apply_dirichlet_dofs_csr_dev: call fh_pattern first");
    if (!values_dev || (n && (!nodes || !components))) return c->fail(FH_BAD_ARGUMENT, "fh_apply_dirichlet_dofs_csr_dev: null pointer");
    const int S = c->S(), N = (int)c->N;
    DevBuf<unsigned char> dm;
    DevBuf<unsigned long long> first;
    DevBuf<double> scale;
    const size_t bytes = ((size_t)N + 4) & ~(size_t)3;
    HIP_TRY(c, dm.alloc(bytes));
    HIP_TRY(c, first.alloc(1));
    HIP_TRY(c, scale.alloc(1));
    HIP_TRY(c, hipMemsetAsync(dm.p, 0, bytes, c->stream));
    uint64_t comp_node[8];
    int rc = dirichlet_masks_to_device(c, "fh_apply_dirichlet_dofs_csr_dev", nodes, components, n, dm.p, comp_node);
    if (!rc) rc = dirichlet_components_fit(c, "fh_apply_dirichlet_dofs_csr_dev", comp_node, S);
    if (rc) return rc;
    HIP_TRY(c, hipMemsetAsync(first.p, 0xff, sizeof(unsigned long long), c->stream));
    const long long R = (long long)N * S;
    hipLaunchKernelGGL(k_first_nonzero_diag, dim3(grid_for(R, 256, 1 << 30)), dim3(256), 0, c->stream, c->noff.p, c->ncols.p, N, S,
                       values_dev, first.p, (double*)nullptr);
    hipLaunchKernelGGL(k_first_nonzero_diag, dim3(1), dim3(64), 0, c->stream, c->noff.p, c->ncols.p, N, S, values_dev, first.p,
                       scale.p);
    if (c->nnz_nodes)
        hipLaunchKernelGGL(k_dirichlet_dof_rows, dim3(grid_for(((long long)N + 7) / 8, 1, 1 << 20)), dim3(256), 0, c->stream, c->noff.p,
                           c->ncols.p, N, S, dm.p, values_dev, scale.p);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the temporaries are released on return)
    return FH_OK;
}

int fh_apply_dirichlet_dofs_rhs_dev(fh_ctx* c, double* rhs_dev, const uint64_t* nodes, const uint8_t* components, uint64_t n) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (!rhs_dev || (n && (!nodes || !components))) return c->fail(FH_BAD_ARGUMENT, "fh_apply_dirichlet_dofs_rhs_dev: null pointer");
    if (n == 0) return FH_OK;
    const int S = c->S();
    uint64_t comp_node[8];
    int rc = dirichlet_masks_to_device(c, "fh_apply_dirichlet_dofs_rhs_dev", nodes, components, n, nullptr, comp_node);
    if (!rc) rc = dirichlet_components_fit(c, "fh_apply_dirichlet_dofs_rhs_dev", comp_node, S);
    if (rc) return rc;
    DevBuf<unsigned long long> dn;
    DevBuf<unsigned char> dc;
    HIP_TRY(c, dn.alloc((size_t)n));
    HIP_TRY(c, dc.alloc((size_t)n));
    HIP_TRY(c, hipMemcpyAsync(dn.p, nodes, sizeof(uint64_t) * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(dc.p, components, n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_dirichlet_dof_rhs, dim3(grid_for((long long)n * S, 256, 1 << 30)), dim3(256), 0, c->stream, rhs_dev, dn.p, dc.p,
                       (long long)n, S);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FH_OK;
}

int fh_apply_dirichlet_rhs_dev(fh_ctx* c, double* rhs_dev, const uint64_t* nodes, uint64_t n) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (!rhs_dev || (n && !nodes)) return c->fail(FH_BAD_ARGUMENT, "fh_apply_dirichlet_rhs_dev: null pointer");
    if (n == 0) return FH_OK;
    for (uint64_t i = 0; i < n; ++i)
        if (nodes[i] >= c->N) return c->fail(FH_BAD_ARGUMENT, "Dirichlet node out of range");
    const int S = c->S();
    DevBuf<unsigned long long> dn;
    HIP_TRY(c, dn.alloc((size_t)n));
    HIP_TRY(c, hipMemcpyAsync(dn.p, nodes, sizeof(uint64_t) * n, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_dirichlet_rhs, dim3(grid_for((long long)n * S, 256, 1 << 30)), dim3(256), 0, c->stream, rhs_dev, dn.p,
                       (long long)n, S);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    return FH_OK;
}

// ---- callers that keep K on the device: CG and the error integrals ---------------------------------
// sum of per-workgroup partials (stride K) in workgroup order: deterministic
extern "C++" int sum_partials(fh_ctx* c, const double* dev, int blocks, int K, double* out) {
    std::vector<double> h((size_t)blocks * K);
    HIP_TRY(c, hipMemcpyAsync(h.data(), dev, sizeof(double) * h.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < K; ++k) {
        double s = 0.0;
        for (int b = 0; b < blocks; ++b) s += h[(size_t)b * K + k];
        out[k] = s;
    }
    return FH_OK;
}

// y = A x (+ the partial sums of x . y, `partials` of them, when `partial` is given).  ONE trip per wavefront: as many short-lived workgroups as the rows need,
// dispatched in order, instead of a resident grid striding over the rows -- the rows in flight stay one compact window of the value array (Hex8
// elasticity 216^3, 19.7 GB of values: 4 096 striding workgroups 5.34 ms, 32 768: 4.99, one trip each (636 k): 4.65; 1 280 = exactly the resident
// ones: 6.7).  The per-workgroup partials of x . y go to `scratch` and are summed over `partials` contiguous ranges in a fixed order.
static int spmv_launch(fh_ctx* c, const double* vals, const double* x, double* y, double* partial, int partials, DevBuf<double>* scratch) {
    const int N = (int)c->N;
    const bool half = c->max_row <= 32 && !c->opt.SPMV_WAVE_PER_NODE;   // half a wavefront per node, one lane per column block
    const int grid = std::max(1, half ? (N + 15) / 16 : (N + 3) / 4);
    double* wg_partial = nullptr;
    if (partial) {
        if (scratch->n < (size_t)grid) HIP_TRY(c, scratch->alloc((size_t)grid));
        wg_partial = scratch->p;
    }
    c->last_kernel = half ? "k_spmv_blocked_half" : "k_spmv_blocked";
    dispatch_or_last(solution_dims, c->S(), [&](auto s) {
        auto kern = half ? k_spmv_blocked_half<s()> : k_spmv_blocked<s()>;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, c->stream, N, c->noff.p, c->ncols.p, vals, x, y, wg_partial);
        return 0;
    });
    HIP_TRY(c, hipGetLastError());
    if (partial) {
        hipLaunchKernelGGL(k_sum_partial_ranges<1>, dim3(partials), dim3(256), 0, c->stream, wg_partial, (long long)grid, partial);
        HIP_TRY(c, hipGetLastError());
    }
    return FH_OK;
}
extern "C++" int csr_spmv(fh_ctx* c, const double* vals, const double* x, double* y) { return spmv_launch(c, vals, x, y, nullptr, 0, nullptr); }
static int matrix_ready(fh_ctx* c, const char* who) {
    if (!c->has_pattern) return c->fail(FH_INVALID_STATE, std::string(who) + ": call fh_pattern first");
    if (c->S() < 1 || c->S() > 3) return c->fail(FH_UNSUPPORTED, std::string(who) + ": solution dim must be 1..3");
    return FH_OK;
}

int fh_spmv_dev(fh_ctx* c, const double* values_dev, const double* x_dev, double* y_dev) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int rc = matrix_ready(c, "fh_spmv");
    if (rc) return rc;
    if (!values_dev || !x_dev || !y_dev) return c->fail(FH_BAD_ARGUMENT, "fh_spmv: null argument");
    if (c->N == 0) return FH_OK;
    return spmv_launch(c, values_dev, x_dev, y_dev, nullptr, 0, nullptr);
}

// ConjugateGradient::solve_with_guess (cg.rs:366-478) around an operator: apply(in, out, ranges) writes out = A in and, when ranges is
// not null, leaves the partials of in . out summed over *ranges contiguous ranges in partial (a DevBuf<double> of at least 3 * max(gv, *ranges)
// doubles: the caller sizes it); dinv: the Jacobi preconditioner or null.  Per iteration the host tests convergence (RelativeResidualCriterion).
// precond (FH_PRECOND_MULTIGRID, dinv null): z = B r as a call of its own after each update of r, and z . r from k_mg_cg_zr.
extern "C++" template <class Apply>
static int cg_run(fh_ctx* c, int n, const double* b_dev, double* x_dev, const double* dinv, DevBuf<double>& partial, DevBuf<double>& wg_partial,
                  double rel_tol, uint64_t max_iter, uint64_t* num_iterations, Apply&& apply,
                  const std::function<int(const double*, double*)>& precond = {}) {
    const int gv = std::min(1024, (n + 255) / 256);                               // vector kernels: ranges of their per-workgroup partials
    const int gvb = std::max(1, (n + 255) / 256);                                 // ... and their workgroups: one entry per thread, short-lived (see spmv_launch)
    DevBuf<double> r, z, p, Ap;
    HIP_TRY(c, r.alloc(n));
    HIP_TRY(c, z.alloc(n));
    HIP_TRY(c, p.alloc(n));
    HIP_TRY(c, Ap.alloc(n));
    if (wg_partial.n < (size_t)3 * gvb) HIP_TRY(c, wg_partial.alloc((size_t)3 * gvb));
    // r = b - A x;  z = P r;  p = z   (cg.rs:388-404)
    int rc = apply(x_dev, r.p, nullptr);
    if (rc) return rc;
    hipLaunchKernelGGL(k_cg_init, dim3(gvb), dim3(256), 0, c->stream, n, b_dev, dinv, r.p, z.p, p.p, wg_partial.p);
    hipLaunchKernelGGL(k_sum_partial_ranges<3>, dim3(gv), dim3(256), 0, c->stream, wg_partial.p, (long long)gvb, partial.p);
    HIP_TRY(c, hipGetLastError());
    double s3[3];
    rc = sum_partials(c, partial.p, gv, 3, s3);
    if (rc) return rc;
    double zTr = s3[0];
    const double b_norm = std::sqrt(s3[1]);
    double r_norm = std::sqrt(s3[2]);
    if (b_norm == 0.0) {  // cg.rs:409-412
        HIP_TRY(c, hipMemsetAsync(x_dev, 0, sizeof(double) * (size_t)n, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return FH_OK;
    }
    if (precond) {   // z = B r, p = z, and z . r
        rc = precond(r.p, z.p);
        if (rc) return rc;
        mg_cg_zr(c->stream, gvb, n, 1, z.p, r.p, p.p, wg_partial.p);
        hipLaunchKernelGGL(k_sum_partial_ranges<1>, dim3(gv), dim3(256), 0, c->stream, wg_partial.p, (long long)gvb, partial.p);
        HIP_TRY(c, hipGetLastError());
        rc = sum_partials(c, partial.p, gv, 1, &zTr);
        if (rc) return rc;
    }
    uint64_t it = 0;
    int status = FH_OK;
    for (;;) {
        if (r_norm <= rel_tol * b_norm) break;  // RelativeResidualCriterion, cg.rs:108-124
        if (max_iter && it >= max_iter) { status = FH_CG_MAX_ITERATIONS; break; }
        double pAp;
        int ranges = 0;
        rc = apply(p.p, Ap.p, &ranges);
        if (rc) return rc;
        rc = sum_partials(c, partial.p, ranges, 1, &pAp);
        if (rc) return rc;
        if (pAp <= 0.0) { status = FH_CG_INDEFINITE_OPERATOR; break; }
        if (zTr <= 0.0) { status = FH_CG_INDEFINITE_PRECONDITIONER; break; }
        const double alpha = zTr / pAp;
        if (precond) {
            mg_cg_update(c->stream, gvb, n, alpha, p.p, Ap.p, x_dev, r.p, wg_partial.p);
            rc = precond(r.p, z.p);
            if (rc) return rc;
            mg_cg_zr(c->stream, gvb, n, 2, z.p, r.p, nullptr, wg_partial.p);
        } else {
            hipLaunchKernelGGL(k_cg_update, dim3(gvb), dim3(256), 0, c->stream, n, alpha, p.p, Ap.p, dinv, x_dev, r.p, z.p, wg_partial.p);
        }
        hipLaunchKernelGGL(k_sum_partial_ranges<2>, dim3(gv), dim3(256), 0, c->stream, wg_partial.p, (long long)gvb, partial.p);
        HIP_TRY(c, hipGetLastError());
        ++it;
        double s2[2];
        rc = sum_partials(c, partial.p, gv, 2, s2);
        if (rc) return rc;
        const double beta = s2[0] / zTr;
        r_norm = std::sqrt(s2[1]);
        hipLaunchKernelGGL(k_cg_direction, dim3(gvb), dim3(256), 0, c->stream, n, beta, z.p, p.p);
        HIP_TRY(c, hipGetLastError());
        zTr = s2[0];
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (num_iterations) *num_iterations = it;
    if (status == FH_CG_MAX_ITERATIONS) return c->fail(status, "CG: max iterations reached");
    if (status == FH_CG_INDEFINITE_OPERATOR) return c->fail(status, "CG: operator appears to be indefinite");
    if (status == FH_CG_INDEFINITE_PRECONDITIONER) return c->fail(status, "CG: indefinite preconditioner");
    return FH_OK;
}

int fh_cg_solve_dev(fh_ctx* c, const double* values_dev, const double* b_dev, double* x_dev, int preconditioner, double rel_tol,
                    uint64_t max_iter, uint64_t* num_iterations) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (num_iterations) *num_iterations = 0;
    int rc = matrix_ready(c, "fh_cg_solve");
    if (rc) return rc;
    if (!values_dev || !b_dev || !x_dev) return c->fail(FH_BAD_ARGUMENT, "fh_cg_solve: null argument");
    if (preconditioner != FH_PRECOND_IDENTITY && preconditioner != FH_PRECOND_JACOBI && preconditioner != FH_PRECOND_AMG)
        return c->fail(FH_BAD_ARGUMENT, "fh_cg_solve: unknown preconditioner");
    const bool amg = preconditioner == FH_PRECOND_AMG;
    if (amg && !c->amg) return c->fail(FH_INVALID_STATE, "fh_cg_solve: FH_PRECOND_AMG needs a hierarchy (fh_set_amg)");
    if (amg && (rc = amg_current(c->amg, "fh_cg_solve"))) return rc;
    const int S = c->S();
    const int n = S * (int)c->N;
    if (n == 0) return FH_OK;
    const int gv = std::min(1024, (n + 255) / 256);
    const int gs = (int)std::min<uint64_t>(2048, (c->N + 3) / 4);                  // SpMV: ranges of its per-workgroup partials
    DevBuf<double> dinv, partial, wg_partial;
    HIP_TRY(c, partial.alloc((size_t)3 * std::max(gv, gs)));
    if (preconditioner == FH_PRECOND_JACOBI) {
        HIP_TRY(c, dinv.alloc(n));
        const int g = (n + 255) / 256;
        dispatch_or_last(solution_dims, S, [&](auto s) {
            hipLaunchKernelGGL((k_inverse_diagonal<s()>), dim3(g), dim3(256), 0, c->stream, (int)c->N, c->noff.p, c->ncols.p, values_dev, dinv.p);
            return 0;
        });
        HIP_TRY(c, hipGetLastError());
    }
    return cg_run(c, n, b_dev, x_dev, dinv.p, partial, wg_partial, rel_tol, max_iter, num_iterations,
                  [&](const double* in, double* out, int* ranges) {
                      if (!ranges) return spmv_launch(c, values_dev, in, out, nullptr, 0, nullptr);
                      *ranges = gs;
                      return spmv_launch(c, values_dev, in, out, partial.p, gs, &wg_partial);
                  },
                  amg ? std::function<int(const double*, double*)>([&](const double* r, double* z) { return amg_precondition(c->amg, r, z); })
                      : std::function<int(const double*, double*)>());
}

// The same solver around the matrix-free map (fh_apply_operator_dev, fh_apply_tangent_dev; scope as mf_ready), or around the shifted map
// alpha M + beta T(u) (fh_apply_shifted_tangent_dev; the plain map is alpha = 0, beta = 1): no pattern, no values.  The partials of p . Ap
// come from the map's node pass (or its last pass off the tiles), summed over at most 2048 ranges in a fixed order; Jacobi takes the
// matrix-free diagonal.  The diagonal (and with it the scale of the Dirichlet rows) is formed once per solve.
extern "C++" int cg_solve_free_dev(fh_ctx* c, const char* who, int scope, const double* b_dev, double* x_dev, int preconditioner, double rel_tol,
                                   uint64_t max_iter, uint64_t* num_iterations, double alpha, double beta) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (num_iterations) *num_iterations = 0;
    int rc = (alpha == 0.0 && beta == 1.0) ? mf_ready(c, who, scope) : mf_shift_ready(c, who, alpha, beta);
    if (rc) return rc;
    if (!b_dev || !x_dev) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null argument");
    if (preconditioner != FH_PRECOND_IDENTITY && preconditioner != FH_PRECOND_JACOBI && preconditioner != FH_PRECOND_MULTIGRID)
        return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": unknown preconditioner");
    const bool multigrid = preconditioner == FH_PRECOND_MULTIGRID;
    if (multigrid && !c->mg) return c->fail(FH_INVALID_STATE, std::string(who) + ": FH_PRECOND_MULTIGRID needs a hierarchy (fh_set_multigrid)");
    MfScope scope_guard_(c, scope);
    if (multigrid && contact_table(c).count)
        return c->fail(FH_UNSUPPORTED, std::string(who) + ": FH_PRECOND_MULTIGRID with obstacles set (fh_set_obstacles): the coarse levels would not see the contact term");
    if (multigrid) {   // (nor the per-element expansion of a hyperelastic operator)
        const int rb = expansion_blocks_multigrid(c, who);
        if (rb) return rb;
    }
    const int S = c->S();
    const int n = S * (int)c->N;
    if (n == 0) return FH_OK;
    const int gv = std::min(1024, (n + 255) / 256);
    const int gs_max = 2048;
    DevBuf<double> dinv, partial, wg_partial;
    HIP_TRY(c, partial.alloc((size_t)3 * std::max(gv, gs_max)));
    if (multigrid) {   // (the fine level's diagonal forms the scale of its Dirichlet rows)
        rc = mg_setup(c, alpha, beta);
        if (rc) return rc;
    } else if (preconditioner == FH_PRECOND_JACOBI || c->mf_num_dirichlet) {
        HIP_TRY(c, dinv.alloc(n));
        rc = mf_shift_diagonal(c, alpha, beta, dinv.p, true);
        if (rc) return rc;
        if (preconditioner == FH_PRECOND_JACOBI) {
            hipLaunchKernelGGL(k_reciprocal, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, dinv.p);
            HIP_TRY(c, hipGetLastError());
        }
    }
    rc = reset_status(c);
    if (rc) return rc;
    const int rcg = cg_run(c, n, b_dev, x_dev, preconditioner == FH_PRECOND_JACOBI ? dinv.p : nullptr, partial, wg_partial, rel_tol, max_iter,
                           num_iterations, [&](const double* in, double* out, int* ranges) {
                               if (!ranges) return mf_shift_apply(c, alpha, beta, in, out, nullptr, nullptr);
                               int count = 0;
                               int r = mf_shift_apply(c, alpha, beta, in, out, &wg_partial, &count);
                               if (r) return r;
                               *ranges = std::min(gs_max, count);
                               hipLaunchKernelGGL(k_sum_partial_ranges<1>, dim3(*ranges), dim3(256), 0, c->stream, wg_partial.p, (long long)count, partial.p);
                               HIP_TRY(c, hipGetLastError());
                               return (int)FH_OK;
                           },
                           multigrid ? std::function<int(const double*, double*)>([&](const double* r, double* z) { return mg_precondition(c, alpha, beta, r, z); })
                                     : std::function<int(const double*, double*)>());
    // a singular Jacobian shows in the map's first application already (and in the diagonal): report it over the solver's status
    rc = read_status(c, nullptr);
    if (rc) return rc;
    if (multigrid) {
        rc = mg_finish(c);
        if (rc) return rc;
    }
    return rcg;
}

int fh_cg_solve_matrix_free_dev(fh_ctx* c, const double* b_dev, double* x_dev, int preconditioner, double rel_tol, uint64_t max_iter,
                                uint64_t* num_iterations) {
    return cg_solve_free_dev(c, "fh_cg_solve_matrix_free", MF_OPERATOR, b_dev, x_dev, preconditioner, rel_tol, max_iter, num_iterations);
}
int fh_cg_solve_tangent_dev(fh_ctx* c, const double* b_dev, double* x_dev, int preconditioner, double rel_tol, uint64_t max_iter,
                            uint64_t* num_iterations) {
    return cg_solve_free_dev(c, "fh_cg_solve_tangent", MF_TANGENT, b_dev, x_dev, preconditioner, rel_tol, max_iter, num_iterations);
}
int fh_cg_solve_shifted_tangent_dev(fh_ctx* c, double alpha, double beta, const double* b_dev, double* x_dev, int preconditioner, double rel_tol,
                                    uint64_t max_iter, uint64_t* num_iterations) {
    return cg_solve_free_dev(c, "fh_cg_solve_shifted_tangent", MF_TANGENT, b_dev, x_dev, preconditioner, rel_tol, max_iter, num_iterations, alpha, beta);
}

int fh_cg_solve(fh_ctx* c, const double* values, const double* b, double* x, int preconditioner, double rel_tol, uint64_t max_iter,
                uint64_t* num_iterations) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int rc = matrix_ready(c, "fh_cg_solve");
    if (rc) return rc;
    if (!values || !b || !x) return c->fail(FH_BAD_ARGUMENT, "fh_cg_solve: null argument");
    const size_t n = (size_t)c->S() * c->N, nnz = (size_t)c->S() * c->S() * c->nnz_nodes;
    DevBuf<double> dv, db, dx;
    HIP_TRY(c, dv.alloc(nnz + 1));
    HIP_TRY(c, db.alloc(n + 1));
    HIP_TRY(c, dx.alloc(n + 1));
    HIP_TRY(c, hipMemcpyAsync(dv.p, values, sizeof(double) * nnz, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(db.p, b, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(dx.p, x, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    rc = fh_cg_solve_dev(c, dv.p, db.p, dx.p, preconditioner, rel_tol, max_iter, num_iterations);
    // like the reference's SolveError, the iterate reached so far is handed back on failure
    HIP_TRY(c, hipMemcpyAsync(x, dx.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return rc;
}

static int cg_solve_free_host(fh_ctx* c, const char* who, int scope, const double* b, double* x, int preconditioner, double rel_tol,
                              uint64_t max_iter, uint64_t* num_iterations, double alpha = 0.0, double beta = 1.0) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (num_iterations) *num_iterations = 0;
    int rc = (alpha == 0.0 && beta == 1.0) ? mf_ready(c, who, scope) : mf_shift_ready(c, who, alpha, beta);
    if (rc) return rc;
    if (!b || !x) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null argument");
    const size_t n = (size_t)c->S() * c->N;
    DevBuf<double> db, dx;
    HIP_TRY(c, db.alloc(n + 1));
    HIP_TRY(c, dx.alloc(n + 1));
    HIP_TRY(c, hipMemcpyAsync(db.p, b, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(dx.p, x, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    rc = cg_solve_free_dev(c, who, scope, db.p, dx.p, preconditioner, rel_tol, max_iter, num_iterations, alpha, beta);
    // like the reference's SolveError, the iterate reached so far is handed back on failure
    HIP_TRY(c, hipMemcpyAsync(x, dx.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return rc;
}

int fh_cg_solve_matrix_free(fh_ctx* c, const double* b, double* x, int preconditioner, double rel_tol, uint64_t max_iter, uint64_t* num_iterations) {
    return cg_solve_free_host(c, "fh_cg_solve_matrix_free", MF_OPERATOR, b, x, preconditioner, rel_tol, max_iter, num_iterations);
}
int fh_cg_solve_tangent(fh_ctx* c, const double* b, double* x, int preconditioner, double rel_tol, uint64_t max_iter, uint64_t* num_iterations) {
    return cg_solve_free_host(c, "fh_cg_solve_tangent", MF_TANGENT, b, x, preconditioner, rel_tol, max_iter, num_iterations);
}
int fh_cg_solve_shifted_tangent(fh_ctx* c, double alpha, double beta, const double* b, double* x, int preconditioner, double rel_tol, uint64_t max_iter,
                                uint64_t* num_iterations) {
    return cg_solve_free_host(c, "fh_cg_solve_shifted_tangent", MF_TANGENT, b, x, preconditioner, rel_tol, max_iter, num_iterations, alpha, beta);
}

static int error_squared(fh_ctx* c, int which, uint32_t sdim, const double* uh_dev, const double* exact_dev, double* out) {
    DevGuard dev_guard_(c->device);
    if (c->rs.active) return c->fail(FH_UNSUPPORTED, "fh_estimate_*_error_squared: rule-set quadrature tables (fh_set_quadrature_rules) are not walked here");
    int rc = source_ready(c, which ? "fh_estimate_H1_seminorm_error_squared" : "fh_estimate_L2_error_squared");
    if (rc) return rc;
    const int D = c->ei.d;
    if (sdim != 1 && (int)sdim != D) return c->fail(FH_BAD_ARGUMENT, "error estimate: solution dim must be 1 or the geometry dim");
    if (!uh_dev || !exact_dev || !out) return c->fail(FH_BAD_ARGUMENT, "error estimate: null argument");
    *out = 0.0;
    if (c->E == 0) return FH_OK;
    rc = reset_status(c);
    if (rc) return rc;
    KArgs a;
    fill_common(c, a);
    SourceArgs sa{};
    sa.N = c->ei.n;
    sa.NG = c->ei.ng;
    sa.phigeom = c->phigeom.p;
    const long long total = (long long)c->E * c->nq;
    const int grid = (int)std::min<long long>(2048, (total + 255) / 256);
    DevBuf<double> partial;
    HIP_TRY(c, partial.alloc(grid));
    dispatch_or_last(int_list<2, 3>{}, D, [&](auto d) {
        return dispatch_bool(sdim == 1, [&](auto scalar) {
            return dispatch_bool(which != 0, [&](auto w) {
                hipLaunchKernelGGL((k_error_squared<d(), scalar() ? 1 : d(), w() ? 1 : 0>), dim3(grid), dim3(256), 0, c->stream, a, sa, uh_dev, exact_dev,
                                   partial.p);
                return 0;
            });
        });
    });
    HIP_TRY(c, hipGetLastError());
    rc = sum_partials(c, partial.p, grid, 1, out);
    if (rc) return rc;
    return which ? read_status(c, nullptr) : FH_OK;
}

static int error_squared_host(fh_ctx* c, int which, uint32_t sdim, const double* uh, const double* exact, double* out) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int rc = source_ready(c, "error estimate");
    if (rc) return rc;
    if (!uh || !exact || !out) return c->fail(FH_BAD_ARGUMENT, "error estimate: null argument");
    const size_t n = (size_t)sdim * c->N, ne = (size_t)c->E * c->nq * sdim * (which ? c->ei.d : 1);
    DevBuf<double> du, de;
    HIP_TRY(c, du.alloc(n + 1));
    HIP_TRY(c, de.alloc(ne + 1));
    HIP_TRY(c, hipMemcpyAsync(du.p, uh, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(de.p, exact, sizeof(double) * ne, hipMemcpyHostToDevice, c->stream));
    return error_squared(c, which, sdim, du.p, de.p, out);
}

int fh_estimate_L2_error_squared(fh_ctx* c, uint32_t sdim, const double* u_h, const double* u_exact, double* out) {
    return c ? error_squared_host(c, 0, sdim, u_h, u_exact, out) : FH_BAD_ARGUMENT;
}
int fh_estimate_L2_error_squared_dev(fh_ctx* c, uint32_t sdim, const double* u_h_dev, const double* u_exact_dev, double* out) {
    return c ? error_squared(c, 0, sdim, u_h_dev, u_exact_dev, out) : FH_BAD_ARGUMENT;
}
int fh_estimate_H1_seminorm_error_squared(fh_ctx* c, uint32_t sdim, const double* u_h, const double* grad_exact, double* out) {
    return c ? error_squared_host(c, 1, sdim, u_h, grad_exact, out) : FH_BAD_ARGUMENT;
}
int fh_estimate_H1_seminorm_error_squared_dev(fh_ctx* c, uint32_t sdim, const double* u_h_dev, const double* grad_exact_dev, double* out) {
    return c ? error_squared(c, 1, sdim, u_h_dev, grad_exact_dev, out) : FH_BAD_ARGUMENT;
}

}  // extern "C"
