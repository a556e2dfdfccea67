// The lowest eigenpairs of T(u) phi = lambda M phi by LOBPCG (fh_eigs_lowest*), and the block-vector layer under it (block_kernels.hpp:
// fh_block_gram_dev, fh_block_combine_dev).  The maps, their diagonal and the V-cycle are the ones of the shifted tangent
// (engine_vector.hip, engine_mg.hip); the small dense problems live on the host (dense_eigh.cpp).
#include "engine_internal.hpp"
#include "block_kernels.hpp"
#include "dense_eigh.hpp"

namespace {

enum EigPhase { EP_MAPS = 0, EP_PRECOND = 1, EP_GRAM = 2, EP_COMBINE = 3, EP_RESIDUAL = 4, EP_DENSE = 5, EP_OTHER = 6, EP_TOTAL = 7 };

struct BlockWork {
    DevBuf<double> partial, out, coef;   // workgroup partials, their sums, the coefficients of a recombination
};

BlockCols cols_of(const double* a, int ca, long long ld, const double* b = nullptr, int cb = 0, const double* d = nullptr, int cd = 0) {
    BlockCols s;
    s.p[0] = a; s.c[0] = ca;
    s.p[1] = b ? b : a; s.c[1] = b ? cb : 0;
    s.p[2] = d ? d : a; s.c[2] = d ? cd : 0;
    s.ld = ld;
    return s;
}

// G (host, p x q row-major) = S^T T over the rows [0, n); the host waits for it
int block_gram(fh_ctx* c, BlockWork& w, int n, const BlockCols& S, const BlockCols& T, const unsigned char* mask, int sdim, double* G) {
    const int p = S.total(), q = T.total(), count = p * q;
    if (n == 0) {
        std::fill(G, G + count, 0.0);
        return FH_OK;
    }
    const int R = BLOCK_GRAM_ROWS;
    int blocks = std::max(1, std::min(1024, (n + 2 * R - 1) / (2 * R)));
    const int per = (((n + blocks - 1) / blocks + R - 1) / R) * R;
    blocks = (n + per - 1) / per;
    if (w.partial.n < (size_t)blocks * count) HIP_TRY(c, w.partial.alloc((size_t)blocks * count));
    if (w.out.n < (size_t)count) HIP_TRY(c, w.out.alloc((size_t)BLOCK_MAX_COLS * BLOCK_MAX_COLS));
    const int widest = std::max(p, q);
    dispatch_or_last(int_list<1, 2, 4, 6>{}, widest <= 16 ? 1 : widest <= 32 ? 2 : widest <= 64 ? 4 : 6, [&](auto a) {
        hipLaunchKernelGGL((k_block_gram<a()>), dim3(blocks), dim3(256), 0, c->stream, n, per, S, T, mask, sdim, w.partial.p);
        return 0;
    });
    hipLaunchKernelGGL(k_block_gram_sum, dim3((count + 255) / 256), dim3(256), 0, c->stream, count, blocks, w.partial.p, w.out.p);
    HIP_TRY(c, hipGetLastError());
    c->last_kernel = "k_block_gram + k_block_gram_sum";
    HIP_TRY(c, hipMemcpyAsync(G, w.out.p, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FH_OK;
}

// Y1 = S C1 (+ Y1) and Y2 = S C2 (+ Y2) with C = [C1 C2] (host, p x (q1 + q2) row-major), q1 + q2 <= BLOCK_COMBINE_MAX_Q; Y2 may be null (q2 = 0)
int block_combine(fh_ctx* c, BlockWork& w, int n, const BlockCols& S, const double* C, int q1, double* Y1, int q2, double* Y2, long long ldy,
                  bool accumulate) {
    const int p = S.total(), qt = q1 + q2;
    if (n == 0 || qt == 0) return FH_OK;
    if (w.coef.n < (size_t)p * qt) HIP_TRY(c, w.coef.alloc((size_t)BLOCK_MAX_COLS * BLOCK_COMBINE_MAX_Q));
    HIP_TRY(c, hipMemcpyAsync(w.coef.p, C, sizeof(double) * p * qt, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // (C belongs to the caller again)
    const int blocks = std::max(1, std::min(1024, (n + 255) / 256));
    const int rc = dispatch_or_last(int_list<8, 16, 32, 64>{}, qt <= 8 ? 8 : qt <= 16 ? 16 : qt <= 32 ? 32 : 64, [&](auto qq) {
        constexpr int Q = qq();
        return launch_lds(c, k_block_combine<Q>, dim3(blocks), dim3(256), sizeof(double) * p * Q, c->stream, n, S, (const double*)w.coef.p, q1, Y1,
                          q2, Y2 ? Y2 : Y1, ldy, accumulate ? 1 : 0);
    });
    c->last_kernel = "k_block_combine";
    return rc;
}

// C (q x q row-major, upper triangular) = L^-T for G = L L^T: the columns of S C are orthonormal in the inner product of the Gram matrix G
bool cholesky_qr_factor(int q, const std::vector<double>& G, std::vector<double>& C) {
    for (double g : G)
        if (!std::isfinite(g)) return false;
    std::vector<double> L;
    if (!dense_cholesky(q, G.data(), L)) return false;
    C.assign((size_t)q * q, 0.0);
    for (int i = 0; i < q; ++i) C[(size_t)i * q + i] = 1.0;
    dense_solve_lower_transposed(q, q, L, C.data());
    return true;
}

struct EigState {
    fh_ctx* c;
    int n, S, m;
    const unsigned char* dmask;
    double shift;
    int precond;
    BlockWork work;
    DevBuf<double> X, KX, MX, Xn, KXn, MXn, W, KW, MW, P, KP, MP, Pn, KPn, MPn, R, T1, dinv, norms_part, norms_out;
    std::vector<double> theta, norms;   // m; 3 m: |R_j|^2, |M x_j|^2, |K x_j|^2
    std::vector<int> act;               // the active columns, ascending
    bool has_P = false;
    uint64_t it = 0, applications = 0, preconditionings = 0, restarts = 0;
    bool prof = false;
    std::chrono::steady_clock::time_point last;

    int lap(int phase) {
        if (!prof) return FH_OK;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        const auto now = std::chrono::steady_clock::now();
        c->eig_profile[phase] += std::chrono::duration<double>(now - last).count();
        last = now;
        return FH_OK;
    }
    double* col(DevBuf<double>& b, int j) { return b.p + (size_t)j * n; }
    int grid() const { return std::max(1, std::min(1024, (n + 255) / 256)); }

    int apply(double alpha, double beta, const double* in, double* out, int cols) {
        for (int j = 0; j < cols; ++j) {
            const int rc = mf_shift_apply(c, alpha, beta, in + (size_t)j * n, out + (size_t)j * n, nullptr, nullptr);
            if (rc) return rc;
            ++applications;
        }
        return lap(EP_MAPS);
    }
    int gram(const BlockCols& A, const BlockCols& B, std::vector<double>& G) {
        G.resize((size_t)A.total() * B.total());
        const int rc = block_gram(c, work, n, A, B, dmask, S, G.data());
        if (rc) return rc;
        return lap(EP_GRAM);
    }
    int combine(const BlockCols& A, const std::vector<double>& C, int q1, double* Y1, int q2, double* Y2, bool accumulate) {
        const int rc = block_combine(c, work, n, A, C.data(), q1, Y1, q2, Y2, n, accumulate);
        if (rc) return rc;
        return lap(EP_COMBINE);
    }
    // B <- B C through the spare block T1 (q columns of B, C q x q)
    int recombine_in_place(DevBuf<double>& B, int q, const std::vector<double>& C) {
        const int rc = combine(cols_of(B.p, q, n), C, q, T1.p, 0, nullptr, false);
        if (rc) return rc;
        part_swap(B, T1);
        return FH_OK;
    }

    // R = K X - theta M X on all m columns and the column norms
    int residuals() {
        BlockScalars th;
        for (int j = 0; j < 32; ++j) th.v[j] = j < m ? theta[j] : 0.0;
        const int g = std::max(1, std::min(256, (n + 255) / 256));
        if (norms_part.n < (size_t)3 * g * m) HIP_TRY(c, norms_part.alloc((size_t)3 * g * m));
        if (norms_out.n < (size_t)3 * m) HIP_TRY(c, norms_out.alloc((size_t)3 * m));
        hipLaunchKernelGGL(k_block_residual, dim3(g, m), dim3(256), 0, c->stream, n, (const double*)KX.p, (const double*)MX.p, (long long)n, th, dmask, S,
                           R.p, norms_part.p);
        hipLaunchKernelGGL(k_block_norm_sum, dim3((3 * m + 255) / 256), dim3(256), 0, c->stream, m, g, (const double*)norms_part.p, norms_out.p);
        HIP_TRY(c, hipGetLastError());
        c->last_kernel = "k_block_residual + k_block_norm_sum";
        norms.resize((size_t)3 * m);
        HIP_TRY(c, hipMemcpyAsync(norms.data(), norms_out.p, sizeof(double) * 3 * m, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return lap(EP_RESIDUAL);
    }

    // fresh K X and M X of the current X, the Rayleigh-Ritz step on span X alone, and X, K X, M X recombined: X is M-orthonormal and theta
    // ascending afterwards.  Both the start and the end of a solve.
    int ritz_on_x() {
        int rc = apply(1.0, 0.0, X.p, MX.p, m);
        if (rc) return rc;
        rc = apply(0.0, 1.0, X.p, KX.p, m);
        if (rc) return rc;
        std::vector<double> A, B, w(m), C((size_t)m * m);
        const BlockCols x = cols_of(X.p, m, n);
        rc = gram(x, cols_of(KX.p, m, n), A);
        if (rc) return rc;
        rc = gram(x, cols_of(MX.p, m, n), B);
        if (rc) return rc;
        rc = fh_dense_generalized_eigh((uint32_t)m, A.data(), B.data(), w.data(), C.data());
        if (rc) return c->fail(rc, "fh_eigs_lowest: the block X is not of full rank in the mass inner product");
        rc = lap(EP_DENSE);
        if (rc) return rc;
        rc = combine(x, C, m, Xn.p, 0, nullptr, false);
        if (rc) return rc;
        rc = combine(cols_of(KX.p, m, n), C, m, KXn.p, 0, nullptr, false);
        if (rc) return rc;
        rc = combine(cols_of(MX.p, m, n), C, m, MXn.p, 0, nullptr, false);
        if (rc) return rc;
        part_swap(X, Xn);
        part_swap(KX, KXn);
        part_swap(MX, MXn);
        theta = w;
        return FH_OK;
    }

    // W = B R on the active columns, zero on the Dirichlet rows
    int precondition() {
        const int na = (int)act.size();
        if (precond == FH_PRECOND_JACOBI) {
            BlockIndex idx;
            for (int a = 0; a < 32; ++a) idx.v[a] = a < na ? act[a] : 0;
            hipLaunchKernelGGL(k_block_jacobi, dim3(grid(), na), dim3(256), 0, c->stream, n, (long long)n, (const double*)dinv.p, (const double*)R.p, idx,
                               dmask, S, W.p);
            HIP_TRY(c, hipGetLastError());
        } else {
            for (int a = 0; a < na; ++a) {
                if (precond == FH_PRECOND_MULTIGRID) {
                    const int rc = mg_precondition(c, shift, 1.0, col(R, act[a]), col(W, a));
                    if (rc) return rc;
                } else {
                    HIP_TRY(c, hipMemcpyAsync(col(W, a), col(R, act[a]), sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
                }
            }
            if (dmask && precond == FH_PRECOND_MULTIGRID) {
                hipLaunchKernelGGL(k_block_mask, dim3(grid(), na), dim3(256), 0, c->stream, n, (long long)n, dmask, S, W.p);
                HIP_TRY(c, hipGetLastError());
            }
        }
        preconditionings += (uint64_t)na;
        return lap(EP_PRECOND);
    }

    // one LOBPCG step on the basis [X W P] (P when has_P).  FH_EIG_BREAKDOWN: a Cholesky factor or the Rayleigh-Ritz step broke down; X, K X,
    // M X, R and theta are then as they were.
    int step() {
        const int na = (int)act.size();
        std::vector<double> G, C;
        int rc = precondition();
        if (rc) return rc;
        // W <- W - X (M X)^T W, then Cholesky-QR in the mass inner product
        rc = gram(cols_of(MX.p, m, n), cols_of(W.p, na, n), G);
        if (rc) return rc;
        for (double& g : G) g = -g;
        rc = combine(cols_of(X.p, m, n), G, na, W.p, 0, nullptr, true);
        if (rc) return rc;
        rc = apply(1.0, 0.0, W.p, MW.p, na);
        if (rc) return rc;
        rc = gram(cols_of(W.p, na, n), cols_of(MW.p, na, n), G);
        if (rc) return rc;
        if (!cholesky_qr_factor(na, G, C)) return FH_EIG_BREAKDOWN;
        rc = recombine_in_place(W, na, C);
        if (rc) return rc;
        rc = recombine_in_place(MW, na, C);
        if (rc) return rc;
        rc = apply(0.0, 1.0, W.p, KW.p, na);
        if (rc) return rc;
        const int np = has_P ? na : 0;
        if (np) {
            rc = gram(cols_of(P.p, np, n), cols_of(MP.p, np, n), G);
            if (rc) return rc;
            if (!cholesky_qr_factor(np, G, C)) return FH_EIG_BREAKDOWN;
            rc = recombine_in_place(P, np, C);
            if (rc) return rc;
            rc = recombine_in_place(KP, np, C);
            if (rc) return rc;
            rc = recombine_in_place(MP, np, C);
            if (rc) return rc;
        }
        // Rayleigh-Ritz on [X W P]
        const int p = m + na + np;
        const BlockCols s = cols_of(X.p, m, n, W.p, na, np ? P.p : nullptr, np);
        const BlockCols ks = cols_of(KX.p, m, n, KW.p, na, np ? KP.p : nullptr, np);
        const BlockCols ms = cols_of(MX.p, m, n, MW.p, na, np ? MP.p : nullptr, np);
        std::vector<double> A, B, w(p), V((size_t)p * p);
        rc = gram(s, ks, A);
        if (rc) return rc;
        rc = gram(s, ms, B);
        if (rc) return rc;
        rc = fh_dense_generalized_eigh((uint32_t)p, A.data(), B.data(), w.data(), V.data());
        if (rc == FH_EIG_BREAKDOWN) return rc;
        if (rc) return c->fail(rc, "fh_eigs_lowest: the Rayleigh-Ritz step failed");
        rc = lap(EP_DENSE);
        if (rc) return rc;
        // the new X = [X W P] V(:, 0:m) and the new P = [W P] V(m:, active columns), from one read of the basis
        const int qt = m + na;
        C.assign((size_t)p * qt, 0.0);
        for (int i = 0; i < p; ++i) {
            for (int j = 0; j < m; ++j) C[(size_t)i * qt + j] = V[(size_t)i * p + j];
            if (i >= m)
                for (int a = 0; a < na; ++a) C[(size_t)i * qt + m + a] = V[(size_t)i * p + act[a]];
        }
        rc = combine(s, C, m, Xn.p, na, Pn.p, false);
        if (rc) return rc;
        rc = combine(ks, C, m, KXn.p, na, KPn.p, false);
        if (rc) return rc;
        rc = combine(ms, C, m, MXn.p, na, MPn.p, false);
        if (rc) return rc;
        part_swap(X, Xn); part_swap(KX, KXn); part_swap(MX, MXn);
        part_swap(P, Pn); part_swap(KP, KPn); part_swap(MP, MPn);
        has_P = true;
        for (int j = 0; j < m; ++j) theta[j] = w[j];
        return FH_OK;
    }

    // the columns of P, K P, M P of the indices in `keep` (a subset of act) moved to the front, in order
    int compact_p(const std::vector<int>& keep) {
        for (size_t a2 = 0; a2 < keep.size(); ++a2) {
            const size_t a = (size_t)(std::find(act.begin(), act.end(), keep[a2]) - act.begin());
            if (a == a2) continue;
            for (DevBuf<double>* b : {&P, &KP, &MP})
                HIP_TRY(c, hipMemcpyAsync(col(*b, (int)a2), col(*b, (int)a), sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
        }
        return FH_OK;
    }
};

// the solve proper: *status is the solver's own outcome (FH_OK, FH_EIG_MAX_ITERATIONS, FH_EIG_BREAKDOWN), the return value an error of the machinery
int eigs_iterate(EigState& e, double tol, uint64_t max_iter, int* status) {
    const int m = e.m;
    *status = FH_OK;
    int rc = e.ritz_on_x();
    if (rc == FH_EIG_BREAKDOWN) { *status = rc; return FH_OK; }
    if (rc) return rc;
    bool fresh = true;   // X, K X, M X and theta come from ritz_on_x
    e.act.resize(m);
    for (int j = 0; j < m; ++j) e.act[j] = j;
    for (;;) {
        rc = e.residuals();
        if (rc) return rc;
        std::vector<int> now;
        for (int j = 0; j < m; ++j) {
            const double bound = tol * (std::fabs(e.theta[j]) + e.shift) * std::sqrt(e.norms[3 * j + 1]);
            if (!(std::sqrt(e.norms[3 * j]) <= bound)) now.push_back(j);
        }
        const bool out_of_steps = !now.empty() && max_iter && e.it >= max_iter;
        if (now.empty() || out_of_steps) {
            if (out_of_steps) *status = FH_EIG_MAX_ITERATIONS;
            if (fresh) return FH_OK;
            rc = e.ritz_on_x();
            if (rc == FH_EIG_BREAKDOWN) { *status = rc; return FH_OK; }
            if (rc) return rc;
            fresh = true;
            if (out_of_steps) return e.residuals();
            continue;   // (the criterion is tested again on the fresh residuals)
        }
        if (e.has_P && now != e.act) {
            if (std::includes(e.act.begin(), e.act.end(), now.begin(), now.end())) {
                rc = e.compact_p(now);
                if (rc) return rc;
            } else {
                e.has_P = false;
            }
        }
        e.act = now;
        rc = e.step();
        if (rc == FH_EIG_BREAKDOWN && e.has_P) {   // once more without P
            e.has_P = false;
            ++e.restarts;
            rc = e.step();
        }
        if (rc == FH_EIG_BREAKDOWN) { *status = rc; return FH_OK; }
        if (rc) return rc;
        ++e.it;
        fresh = false;
    }
}

int eigs_lowest_dev(fh_ctx* c, uint32_t m32, double shift, int preconditioner, double tol, uint64_t max_iter, int use_guess, double* X_dev,
                    double* theta, double* residual_norms, uint64_t* stats) {
    const char* who = "fh_eigs_lowest";
    if (stats) std::fill(stats, stats + 4, (uint64_t)0);
    const FrictionOff no_friction(c);   // (the friction block of fh_set_friction stays out of the pencil)
    int rc = mf_ready(c, who, MF_TANGENT);
    if (rc) return rc;
    if (!X_dev || !theta) return c->fail(FH_BAD_ARGUMENT, "fh_eigs_lowest: null argument");
    if (m32 == 0 || m32 > FH_EIG_MAX_BLOCK) return c->fail(FH_BAD_ARGUMENT, "fh_eigs_lowest: m must be 1..FH_EIG_MAX_BLOCK");
    if (!std::isfinite(shift) || shift < 0.0) return c->fail(FH_BAD_ARGUMENT, "fh_eigs_lowest: shift must be finite and >= 0");
    if (!std::isfinite(tol)) return c->fail(FH_BAD_ARGUMENT, "fh_eigs_lowest: tol must be finite");
    if (preconditioner != FH_PRECOND_IDENTITY && preconditioner != FH_PRECOND_JACOBI && preconditioner != FH_PRECOND_MULTIGRID)
        return c->fail(FH_BAD_ARGUMENT, "fh_eigs_lowest: unknown preconditioner");
    if (c->mass_rho_n == 0) return c->fail(FH_INVALID_STATE, "fh_eigs_lowest: the mass needs fh_set_mass_density");
    const bool multigrid = preconditioner == FH_PRECOND_MULTIGRID;
    if (multigrid && !c->mg) return c->fail(FH_INVALID_STATE, "fh_eigs_lowest: FH_PRECOND_MULTIGRID needs a hierarchy (fh_set_multigrid)");
    if (multigrid && contact_table(c).count)
        return c->fail(FH_UNSUPPORTED, "fh_eigs_lowest: FH_PRECOND_MULTIGRID with obstacles set (fh_set_obstacles): the coarse levels would not see the contact term");
    if (multigrid) {   // (nor the per-element expansion of a hyperelastic operator)
        const int rb = expansion_blocks_multigrid(c, "fh_eigs_lowest");
        if (rb) return rb;
    }
    if ((uint64_t)c->S() * c->N >= (1ull << 31)) return c->fail(FH_UNSUPPORTED, "fh_eigs_lowest: more than 2^31 - 1 dofs");
    EigState e;
    e.c = c;
    e.S = c->S();
    e.n = e.S * (int)c->N;
    e.m = (int)m32;
    e.shift = shift;
    e.precond = preconditioner;
    e.dmask = c->mf_num_dirichlet ? c->mf_dmask.p : nullptr;
    uint64_t free_dofs = (uint64_t)e.S * c->N;
    if (e.dmask) {
        std::vector<unsigned char> h(c->N);
        HIP_TRY(c, hipMemcpyAsync(h.data(), c->mf_dmask.p, c->N, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        for (uint64_t i = 0; i < c->N; ++i)
            for (int k = 0; k < e.S; ++k) free_dofs -= dof_fixed(h.data(), i, k) ? 1u : 0u;
    }
    if ((uint64_t)e.m * 3 > free_dofs) return c->fail(FH_BAD_ARGUMENT, "fh_eigs_lowest: m must not exceed a third of the free dofs");
    const int n = e.n, m = e.m;
    const size_t block = (size_t)n * m;
    for (DevBuf<double>* b : {&e.X, &e.KX, &e.MX, &e.Xn, &e.KXn, &e.MXn, &e.W, &e.KW, &e.MW, &e.P, &e.KP, &e.MP, &e.Pn, &e.KPn, &e.MPn, &e.R, &e.T1})
        if (b->alloc(block) != hipSuccess) return c->fail(FH_OUT_OF_MEMORY, "fh_eigs_lowest: the block vectors (17 n m doubles) do not fit");
    // the preconditioner of shift M + T(u); its diagonal also forms the scale of the Dirichlet rows the maps read
    if (multigrid) {
        rc = mg_setup(c, shift, 1.0);
        if (rc) return rc;
    } else if (preconditioner == FH_PRECOND_JACOBI || e.dmask) {
        HIP_TRY(c, e.dinv.alloc(n));
        rc = mf_shift_diagonal(c, shift, 1.0, e.dinv.p, true);
        if (rc) return rc;
        if (preconditioner == FH_PRECOND_JACOBI) {
            hipLaunchKernelGGL(k_reciprocal, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, e.dinv.p);
            HIP_TRY(c, hipGetLastError());
        }
    }
    rc = reset_status(c);
    if (rc) return rc;
    e.prof = c->opt.EIGS_PROFILE;
    std::fill(c->eig_profile, c->eig_profile + 8, 0.0);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const auto t0 = std::chrono::steady_clock::now();
    e.last = t0;
    if (use_guess) {
        HIP_TRY(c, hipMemcpyAsync(e.X.p, X_dev, sizeof(double) * block, hipMemcpyDeviceToDevice, c->stream));
        if (e.dmask) hipLaunchKernelGGL(k_block_mask, dim3(e.grid(), m), dim3(256), 0, c->stream, n, (long long)n, e.dmask, e.S, e.X.p);
    } else {
        hipLaunchKernelGGL(k_block_fill, dim3(e.grid(), m), dim3(256), 0, c->stream, n, (long long)n, e.dmask, e.S, e.X.p);
    }
    HIP_TRY(c, hipGetLastError());
    rc = e.lap(EP_OTHER);
    if (rc) return rc;
    int status = FH_OK;
    const int rci = eigs_iterate(e, tol, max_iter, &status);
    if (stats) {
        stats[0] = e.it;
        stats[1] = e.applications;
        stats[2] = e.preconditionings;
        stats[3] = e.restarts;
    }
    // a singular Jacobian shows in the map's first application already: report it over the solver's status
    rc = read_status(c, nullptr);
    if (rc) return rc;
    if (multigrid) {
        rc = mg_finish(c);
        if (rc) return rc;
    }
    if (rci) return rci;
    // the pairs reached so far are handed back, whatever the status
    HIP_TRY(c, hipMemcpyAsync(X_dev, e.X.p, sizeof(double) * block, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int j = 0; j < m; ++j) {
        theta[j] = e.theta.size() == (size_t)m ? e.theta[j] : 0.0;
        if (residual_norms) residual_norms[j] = e.norms.size() == (size_t)3 * m ? std::sqrt(e.norms[3 * j]) : 0.0;
    }
    c->eig_profile[EP_TOTAL] = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (status == FH_EIG_MAX_ITERATIONS) return c->fail(status, "fh_eigs_lowest: max iterations reached");
    if (status == FH_EIG_BREAKDOWN) return c->fail(status, "fh_eigs_lowest: the basis lost its rank (Cholesky or Rayleigh-Ritz breakdown)");
    return FH_OK;
}

bool ranges_overlap(const double* a, size_t na, const double* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + na * sizeof(double), b0 = (uintptr_t)b, b1 = b0 + nb * sizeof(double);
    return a0 < b1 && b0 < a1;
}

}  // namespace

extern "C" {

int fh_block_gram_dev(fh_ctx* c, uint64_t n, uint32_t p, const double* S_dev, uint64_t lds, uint32_t q, const double* T_dev, uint64_t ldt,
                      double* G) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (!S_dev || !T_dev || !G) return c->fail(FH_BAD_ARGUMENT, "fh_block_gram_dev: null argument");
    if (p == 0 || p > (uint32_t)BLOCK_MAX_COLS || q == 0 || q > (uint32_t)BLOCK_MAX_COLS)
        return c->fail(FH_BAD_ARGUMENT, "fh_block_gram_dev: p and q must be 1..96");
    if (lds < n || ldt < n) return c->fail(FH_BAD_ARGUMENT, "fh_block_gram_dev: a leading dimension is below n");
    if (n >= (1ull << 31)) return c->fail(FH_BAD_ARGUMENT, "fh_block_gram_dev: n must be below 2^31");
    BlockWork w;
    return block_gram(c, w, (int)n, cols_of(S_dev, (int)p, (long long)lds), cols_of(T_dev, (int)q, (long long)ldt), nullptr, 1, G);
}

int fh_block_combine_dev(fh_ctx* c, uint64_t n, uint32_t p, const double* S_dev, uint64_t lds, uint32_t q, const double* C, double* Y_dev,
                         uint64_t ldy, int accumulate) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (!S_dev || !C || !Y_dev) return c->fail(FH_BAD_ARGUMENT, "fh_block_combine_dev: null argument");
    if (p == 0 || p > (uint32_t)BLOCK_MAX_COLS || q == 0 || q > (uint32_t)BLOCK_MAX_COLS)
        return c->fail(FH_BAD_ARGUMENT, "fh_block_combine_dev: p and q must be 1..96");
    if (lds < n || ldy < n) return c->fail(FH_BAD_ARGUMENT, "fh_block_combine_dev: a leading dimension is below n");
    if (n >= (1ull << 31)) return c->fail(FH_BAD_ARGUMENT, "fh_block_combine_dev: n must be below 2^31");
    if (n == 0) return FH_OK;
    if (ranges_overlap(S_dev, (size_t)(p - 1) * lds + n, Y_dev, (size_t)(q - 1) * ldy + n))
        return c->fail(FH_BAD_ARGUMENT, "fh_block_combine_dev: Y may not overlap S");
    BlockWork w;
    std::vector<double> part;
    for (uint32_t j0 = 0; j0 < q; j0 += (uint32_t)BLOCK_COMBINE_MAX_Q) {   // (more than 64 output columns: S is read once per 64 of them)
        const int qb = (int)std::min<uint32_t>((uint32_t)BLOCK_COMBINE_MAX_Q, q - j0);
        part.resize((size_t)p * qb);
        for (uint32_t i = 0; i < p; ++i)
            for (int j = 0; j < qb; ++j) part[(size_t)i * qb + j] = C[(size_t)i * q + j0 + j];
        const int rc = block_combine(c, w, (int)n, cols_of(S_dev, (int)p, (long long)lds), part.data(), qb, Y_dev + (size_t)j0 * ldy, 0, nullptr,
                                     (long long)ldy, accumulate != 0);
        if (rc) return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the scratch is released on return)
    return FH_OK;
}

int fh_eigs_lowest_dev(fh_ctx* c, uint32_t m, double shift, int preconditioner, double tol, uint64_t max_iter, int use_guess, double* X_dev,
                       double* theta, double* residual_norms, uint64_t* stats) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    return eigs_lowest_dev(c, m, shift, preconditioner, tol, max_iter, use_guess, X_dev, theta, residual_norms, stats);
}

int fh_eigs_lowest(fh_ctx* c, uint32_t m, double shift, int preconditioner, double tol, uint64_t max_iter, int use_guess, double* X, double* theta,
                   double* residual_norms, uint64_t* stats) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (stats) std::fill(stats, stats + 4, (uint64_t)0);
    if (!X || !theta) return c->fail(FH_BAD_ARGUMENT, "fh_eigs_lowest: null argument");
    const size_t count = (size_t)c->S() * c->N * std::min<uint32_t>(m, FH_EIG_MAX_BLOCK);
    DevBuf<double> dx;
    HIP_TRY(c, dx.alloc(count + 1));
    if (use_guess && count) {
        HIP_TRY(c, hipMemcpyAsync(dx.p, X, sizeof(double) * count, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    const int rc = eigs_lowest_dev(c, m, shift, preconditioner, tol, max_iter, use_guess, dx.p, theta, residual_norms, stats);
    if (rc == FH_OK || rc == FH_EIG_MAX_ITERATIONS || rc == FH_EIG_BREAKDOWN) {
        const std::string msg = c->err;
        HIP_TRY(c, hipMemcpyAsync(X, dx.p, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->err = msg;
    }
    return rc;
}

int fh_eigs_profile(fh_ctx* c, double* seconds) {
    if (!c) return FH_BAD_ARGUMENT;
    if (!seconds) return c->fail(FH_BAD_ARGUMENT, "fh_eigs_profile: null argument");
    std::copy(c->eig_profile, c->eig_profile + 8, seconds);
    return FH_OK;
}

}  // extern "C"
