// Geometric multigrid over a hierarchy of contexts (fh_mg): a V-cycle on alpha M + beta T(u) at every level through each level's own
// matrix-free map and diagonal, used as the preconditioner of the matrix-free PCG (FH_PRECOND_MULTIGRID) and as fh_mg_apply_dev.
//
// Levels: lv[0] is the coarsest, lv[L] the fine context.  The transfer of pair l (lv[l - 1] -> lv[l]) lives on lv[l]: P as CSR by fine node
// (at most 8 parents), its transpose R as CSR by coarse node in ascending fine index, and the injection (coarse node -> its fine copy).
// Streams: every call runs on the fine context's stream; the coarse contexts' stream slots are pointed at it for the duration of the call
// (StreamBorrow) and given back on return, so all of a V-cycle's work is ordered on one stream with no host synchronisation inside it.
#include <memory>

#include "engine_internal.hpp"
#include "mg_kernels.hpp"

using namespace fenris_hip_mg;

namespace {
constexpr int MG_MAX_COARSE_DOFS = 4096;

struct MgLevel {
    fh_ctx* c = nullptr;
    int S = 0, N = 0, n = 0;
    unsigned long long topo_gen = 0;   // the level's mesh at creation: the vectors and transfers below have its sizes
    DevBuf<double> diag, b, x, r, d, t;
    double lambda = 0.0;
    unsigned long long key[8] = {};
    bool have_key = false;
    DevBuf<unsigned> p_off, p_idx, r_off, r_idx, inj;
    DevBuf<double> p_w, r_w;
    const unsigned char* dmask() const { return c->mf_num_dirichlet ? c->mf_dmask.p : nullptr; }
};
}  // namespace

struct fh_mg {
    fh_ctx* fine = nullptr;   // null once the fine context was destroyed (fh_destroy orphans an attached hierarchy)
    int device = 0;
    std::vector<MgLevel> lv;
    uint32_t degree = 3, eig_steps = 10;
    double range = 15.0;
    DevBuf<double> ainv;   // coarsest level: the dense inverse, row-major
};

namespace {
// what the diagonal, the eigenvalue estimate and the coarse factor depend on: the key of the Dirichlet scale (mf_scale_key_now,
// engine_vector.hip) and the Dirichlet set
void mg_key(const fh_ctx* c, double alpha, double beta, unsigned long long (&k)[8]) {
    k[0] = c->struct_gen;
    k[1] = c->topo_gen;
    k[2] = c->geom_gen;
    k[3] = (c->op <= FH_LINEAR_ELASTIC || beta == 0.0) ? 0 : c->u_gen;
    std::memcpy(&k[4], &alpha, sizeof(double));
    std::memcpy(&k[5], &beta, sizeof(double));
    k[6] = alpha != 0.0 ? c->density_gen : 0;
    k[7] = c->dirichlet_gen;
}

struct StreamBorrow {
    fh_mg* mg;
    std::vector<hipStream_t> saved;
    explicit StreamBorrow(fh_mg* m) : mg(m) {
        for (auto& l : mg->lv) {
            saved.push_back(l.c->stream);
            l.c->stream = mg->fine->stream;
        }
    }
    ~StreamBorrow() {
        for (size_t i = 0; i < saved.size(); ++i) mg->lv[i].c->stream = saved[i];
    }
};

int apply_level(MgLevel& L, double alpha, double beta, const double* x, double* y) {
    return mf_shift_apply(L.c, alpha, beta, x, y, nullptr, nullptr);
}

// largest eigenvalue of the k x k symmetric tridiagonal (a: diagonal, b: off-diagonal) by Sturm bisection
double tridiag_max_eig(const std::vector<double>& a, const std::vector<double>& b) {
    const size_t k = a.size();
    double lo = 0.0, hi = 0.0;
    for (size_t i = 0; i < k; ++i) {
        const double r = (i ? std::fabs(b[i - 1]) : 0.0) + (i + 1 < k ? std::fabs(b[i]) : 0.0);
        lo = i ? std::min(lo, a[i] - r) : a[i] - r;
        hi = i ? std::max(hi, a[i] + r) : a[i] + r;
    }
    auto count_below = [&](double x) {   // eigenvalues < x
        int cnt = 0;
        double q = 1.0;
        for (size_t i = 0; i < k; ++i) {
            q = a[i] - x - (i ? b[i - 1] * b[i - 1] / q : 0.0);
            if (q == 0.0) q = -1e-300;
            if (q < 0.0) ++cnt;
        }
        return cnt;
    };
    for (int it = 0; it < 200 && hi - lo > 1e-14 * std::max(1.0, std::fabs(hi)); ++it) {
        const double mid = 0.5 * (lo + hi);
        if (count_below(mid) >= (int)k) hi = mid; else lo = mid;
    }
    return hi;
}

}  // namespace

// lambda_max of D^-1 A: eig_steps steps of Jacobi-PCG from the fixed start vector, the Lanczos tridiagonal of their coefficients.  apply
// writes y = A x and the per-workgroup partials of x . y (*count of them) into *dots; diag: the point diagonal; dmask: S-blocks left at 0
// in the start vector (or null).  Shared with the algebraic hierarchy (engine_amg.hip).
extern "C++" int mg_estimate_lambda(fh_ctx* f, hipStream_t st, int n, int S, const unsigned char* dmask, const double* diag, uint32_t eig_steps,
                                    const LevelApply& apply, const char* who, double* lambda) {
    const int gvb = std::max(1, (n + 255) / 256), gv = std::min(1024, gvb);
    DevBuf<double> v, r, z, p, Ap, x, dinv, partial, wg, dots;
    HIP_TRY(f, v.alloc(n));
    HIP_TRY(f, r.alloc(n));
    HIP_TRY(f, z.alloc(n));
    HIP_TRY(f, p.alloc(n));
    HIP_TRY(f, Ap.alloc(n));
    HIP_TRY(f, x.alloc(n));
    HIP_TRY(f, dinv.alloc(n));
    HIP_TRY(f, partial.alloc((size_t)3 * 2048));
    HIP_TRY(f, wg.alloc((size_t)3 * gvb));
    HIP_TRY(f, hipMemcpyAsync(dinv.p, diag, sizeof(double) * n, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_reciprocal, dim3(gvb), dim3(256), 0, st, n, dinv.p);
    hipLaunchKernelGGL(k_mg_start_vector, dim3(gvb), dim3(256), 0, st, n, S, dmask, v.p);
    HIP_TRY(f, hipMemsetAsync(r.p, 0, sizeof(double) * n, st));   // A x for x = 0
    HIP_TRY(f, hipMemsetAsync(x.p, 0, sizeof(double) * n, st));
    hipLaunchKernelGGL(k_cg_init, dim3(gvb), dim3(256), 0, st, n, v.p, dinv.p, r.p, z.p, p.p, wg.p);
    hipLaunchKernelGGL(k_sum_partial_ranges<3>, dim3(gv), dim3(256), 0, st, wg.p, (long long)gvb, partial.p);
    HIP_TRY(f, hipGetLastError());
    double s3[3];
    int rc = sum_partials(f, partial.p, gv, 3, s3);
    if (rc) return rc;
    double zTr = s3[0];
    std::vector<double> alphas, betas;
    for (uint32_t k = 0; k < eig_steps; ++k) {
        if (!(zTr > 0.0)) break;
        int count = 0;
        rc = apply(p.p, Ap.p, &dots, &count);
        if (rc) return rc;
        const int ranges = std::min(2048, count);
        hipLaunchKernelGGL(k_sum_partial_ranges<1>, dim3(ranges), dim3(256), 0, st, dots.p, (long long)count, partial.p);
        HIP_TRY(f, hipGetLastError());
        double pAp;
        rc = sum_partials(f, partial.p, ranges, 1, &pAp);
        if (rc) return rc;
        if (!(pAp > 0.0)) {
            if (alphas.empty()) return f->fail(FH_CG_INDEFINITE_PRECONDITIONER, std::string(who) + ": a level's operator is not positive definite");
            break;
        }
        const double a = zTr / pAp;
        alphas.push_back(a);
        hipLaunchKernelGGL(k_cg_update, dim3(gvb), dim3(256), 0, st, n, a, p.p, Ap.p, dinv.p, x.p, r.p, z.p, wg.p);
        hipLaunchKernelGGL(k_sum_partial_ranges<2>, dim3(gv), dim3(256), 0, st, wg.p, (long long)gvb, partial.p);
        HIP_TRY(f, hipGetLastError());
        double s2[2];
        rc = sum_partials(f, partial.p, gv, 2, s2);
        if (rc) return rc;
        const double bt = s2[0] / zTr;
        zTr = s2[0];
        if (k + 1 == eig_steps || !(zTr > 0.0)) break;
        betas.push_back(bt);
        hipLaunchKernelGGL(k_cg_direction, dim3(gvb), dim3(256), 0, st, n, bt, z.p, p.p);
        HIP_TRY(f, hipGetLastError());
    }
    if (alphas.empty()) return f->fail(FH_CG_INDEFINITE_PRECONDITIONER, std::string(who) + ": no eigenvalue estimate for a level");
    const size_t k = alphas.size();
    std::vector<double> ta(k), tb(k > 1 ? k - 1 : 0);
    for (size_t i = 0; i < k; ++i) {
        ta[i] = 1.0 / alphas[i] + (i ? betas[i - 1] / alphas[i - 1] : 0.0);
        if (i + 1 < k) tb[i] = std::sqrt(betas[i]) / alphas[i];
    }
    *lambda = tridiag_max_eig(ta, tb);
    HIP_TRY(f, hipStreamSynchronize(st));   // (the temporaries are released on return)
    return FH_OK;
}

namespace {
int estimate_lambda(fh_mg* mg, MgLevel& L, double alpha, double beta) {
    fh_ctx* c = L.c;
    return mg_estimate_lambda(mg->fine, c->stream, L.n, L.S, L.dmask(), L.diag.p, mg->eig_steps,
                              [&](const double* x, double* y, DevBuf<double>* dots, int* count) { return mf_shift_apply(c, alpha, beta, x, y, dots, count); },
                              "multigrid", &L.lambda);
}

}  // namespace

// The inverse of the dense symmetric n x n matrix A (row-major; A is overwritten): Cholesky A = L L^T on the host, W = L^-1, Ainv = W^T W,
// exactly symmetric.  Not SPD: FH_CG_INDEFINITE_PRECONDITIONER.  drop > 0: a pivot at most drop times its diagonal leaves that dof out
// (its rows of the inverse are zero), for semidefinite matrices.  Shared with the algebraic hierarchy (engine_amg.hip).
extern "C++" int mg_dense_inverse(fh_ctx* f, const char* who, std::vector<double>& A, int n, std::vector<double>& Ainv, double drop) {
    std::vector<char> dropped(n, 0);
    std::vector<double> d0;
    if (drop > 0.0)
        for (int j = 0; j < n; ++j) d0.push_back(A[(size_t)j * n + j]);
    // Cholesky A = L L^T, lower triangle in place
    for (int j = 0; j < n; ++j) {
        double* rj = &A[(size_t)j * n];
        double s = rj[j];
        for (int k = 0; k < j; ++k) s -= rj[k] * rj[k];
        if (drop > 0.0 && std::isfinite(s) && s <= drop * d0[j]) {   // (semidefinite: the dof is left out)
            dropped[j] = 1;
            for (int i = j; i < n; ++i) A[(size_t)i * n + j] = 0.0;
            continue;
        }
        if (!(s > 0.0) || !std::isfinite(s))
            return f->fail(FH_CG_INDEFINITE_PRECONDITIONER, std::string(who) + ": the coarsest level's matrix is not positive definite");
        const double djj = std::sqrt(s);
        rj[j] = djj;
        for (int i = j + 1; i < n; ++i) {
            double* ri = &A[(size_t)i * n];
            double t = ri[j];
            for (int k = 0; k < j; ++k) t -= ri[k] * rj[k];
            ri[j] = t / djj;
        }
    }
    // W = L^-1 (lower), row-major; Ainv = W^T W, exactly symmetric
    std::vector<double> W((size_t)n * n, 0.0);
    for (int col = 0; col < n; ++col) {
        if (dropped[col]) continue;
        W[(size_t)col * n + col] = 1.0 / A[(size_t)col * n + col];
        for (int i = col + 1; i < n; ++i) {
            if (dropped[i]) continue;
            double t = 0.0;
            for (int k = col; k < i; ++k) t += A[(size_t)i * n + k] * W[(size_t)k * n + col];
            W[(size_t)i * n + col] = -t / A[(size_t)i * n + i];
        }
    }
    Ainv.assign((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i)
        for (int j = i; j < n; ++j) {
            double t = 0.0;
            for (int k = j; k < n; ++k) t += W[(size_t)k * n + i] * W[(size_t)k * n + j];
            Ainv[(size_t)i * n + j] = Ainv[(size_t)j * n + i] = t;
        }
    return FH_OK;
}

namespace {
// the coarsest level's dense matrix through its map, probed with a distance-2 colouring of its nodes; Cholesky on the host; the inverse
// W^T W (W = L^-1) uploaded.  Not SPD: FH_CG_INDEFINITE_PRECONDITIONER.
int factor_coarsest(fh_mg* mg, MgLevel& L, double alpha, double beta) {
    fh_ctx* c = L.c;
    fh_ctx* f = mg->fine;
    const int S = L.S, N = L.N, n = L.n, nen = c->ei.n;
    const uint64_t E = c->E;
    std::vector<int> conn((size_t)E * nen);
    if (E) HIP_TRY(f, hipMemcpyAsync(conn.data(), c->conn.p, sizeof(int) * conn.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(f, hipStreamSynchronize(c->stream));
    std::vector<std::vector<int>> adj(N);
    for (uint64_t e = 0; e < E; ++e)
        for (int a = 0; a < nen; ++a)
            for (int b = 0; b < nen; ++b) adj[conn[(size_t)e * nen + a]].push_back(conn[(size_t)e * nen + b]);
    for (int i = 0; i < N; ++i) {
        adj[i].push_back(i);
        std::sort(adj[i].begin(), adj[i].end());
        adj[i].erase(std::unique(adj[i].begin(), adj[i].end()), adj[i].end());
    }
    std::vector<int> color(N, -1), stamp;
    int ncol = 0;
    for (int j = 0; j < N; ++j) {
        stamp.assign((size_t)ncol + 1, 0);
        for (int i : adj[j])
            for (int k : adj[i])
                if (color[k] >= 0) stamp[color[k]] = 1;
        int cc = 0;
        while (stamp[cc]) ++cc;
        color[j] = cc;
        ncol = std::max(ncol, cc + 1);
    }
    const int probes = ncol * S;
    std::vector<double> X((size_t)probes * n, 0.0), Y((size_t)probes * n);
    for (int j = 0; j < N; ++j)
        for (int s = 0; s < S; ++s) X[(size_t)(color[j] * S + s) * n + (size_t)S * j + s] = 1.0;
    DevBuf<double> dX, dY;
    HIP_TRY(f, dX.alloc(X.size()));
    HIP_TRY(f, dY.alloc(Y.size()));
    HIP_TRY(f, hipMemcpyAsync(dX.p, X.data(), sizeof(double) * X.size(), hipMemcpyHostToDevice, c->stream));
    for (int q = 0; q < probes; ++q) {
        const int rc = apply_level(L, alpha, beta, dX.p + (size_t)q * n, dY.p + (size_t)q * n);
        if (rc) return rc;
    }
    HIP_TRY(f, hipMemcpyAsync(Y.data(), dY.p, sizeof(double) * Y.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(f, hipStreamSynchronize(c->stream));
    std::vector<double> A((size_t)n * n, 0.0);
    for (int i = 0; i < N; ++i)
        for (int a = 0; a < S; ++a)
            for (int j : adj[i])
                for (int s = 0; s < S; ++s)
                    A[(size_t)(S * i + a) * n + S * j + s] = Y[(size_t)(color[j] * S + s) * n + (size_t)S * i + a];
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            const double m = 0.5 * (A[(size_t)i * n + j] + A[(size_t)j * n + i]);
            A[(size_t)i * n + j] = A[(size_t)j * n + i] = m;
        }
    std::vector<double> Ainv;
    const int rc = mg_dense_inverse(f, "multigrid", A, n, Ainv);
    if (rc) return rc;
    if (mg->ainv.n < (size_t)n * n) HIP_TRY(f, mg->ainv.alloc((size_t)n * n));
    HIP_TRY(f, hipMemcpyAsync(mg->ainv.p, Ainv.data(), sizeof(double) * Ainv.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(f, hipStreamSynchronize(c->stream));
    return FH_OK;
}

}  // namespace

// Chebyshev-Jacobi smoothing of degree `degree` on x (the recurrence of fenris_hip.h) with apply = the level's operator (dots null); r, d, t:
// the level's work vectors.  Shared with the algebraic hierarchy (engine_amg.hip).
extern "C++" int mg_chebyshev(hipStream_t st, const LevelApply& apply, int n, const double* diag, double lambda, uint32_t degree, double range,
                              double* r, double* d, double* t, const double* b, double* x, bool zero_start) {
    const int g = grid_for(n, 256);
    const double hi = 1.1 * lambda, lo = lambda / range;
    const double theta = 0.5 * (hi + lo), delta = 0.5 * (hi - lo);
    int rc;
    if (zero_start) {
        hipLaunchKernelGGL(k_mg_cheb_start, dim3(g), dim3(256), 0, st, n, b, (const double*)nullptr, diag, 1.0 / theta, x, r, d);
    } else {
        rc = apply(x, t, nullptr, nullptr);
        if (rc) return rc;
        hipLaunchKernelGGL(k_mg_cheb_start, dim3(g), dim3(256), 0, st, n, b, (const double*)t, diag, 1.0 / theta, (double*)nullptr, r, d);
    }
    double rho = delta / theta;
    for (uint32_t k = 1; k <= degree; ++k) {
        if (k < degree) {
            rc = apply(d, t, nullptr, nullptr);
            if (rc) return rc;
            const double rho1 = 1.0 / (2.0 * theta / delta - rho);
            hipLaunchKernelGGL(k_mg_cheb_step, dim3(g), dim3(256), 0, st, n, (const double*)t, diag, rho1 * rho, 2.0 * rho1 / delta, x, r, d);
            rho = rho1;
        } else {
            hipLaunchKernelGGL(k_mg_add, dim3(g), dim3(256), 0, st, n, (const double*)d, x);
        }
    }
    return FH_OK;
}

namespace {
int chebyshev(fh_mg* mg, MgLevel& L, double alpha, double beta, const double* b, double* x, bool zero_start) {
    return mg_chebyshev(mg->fine->stream,
                        [&](const double* in, double* out, DevBuf<double>*, int*) { return apply_level(L, alpha, beta, in, out); }, L.n,
                        L.diag.p, L.lambda, mg->degree, mg->range, L.r.p, L.d.p, L.t.p, b, x, zero_start);
}

int vcycle(fh_mg* mg, int l, double alpha, double beta, const double* b, double* x) {
    MgLevel& L = mg->lv[l];
    hipStream_t st = mg->fine->stream;
    const int n = L.n;
    const unsigned char* dm = L.dmask();
    int rc;
    if (l == 0) {
        hipLaunchKernelGGL(k_mg_dense_apply, dim3((n + 3) / 4), dim3(256), 0, st, n, (const double*)mg->ainv.p, b, x);
    } else {
        MgLevel& C = mg->lv[l - 1];
        rc = chebyshev(mg, L, alpha, beta, b, x, true);
        if (rc) return rc;
        rc = apply_level(L, alpha, beta, x, L.t.p);
        if (rc) return rc;
        hipLaunchKernelGGL(k_mg_restrict_residual, dim3(grid_for(C.n, 256)), dim3(256), 0, st, C.N, C.S, (const unsigned*)L.r_off.p,
                           (const unsigned*)L.r_idx.p, (const double*)L.r_w.p, dm, C.dmask(), b, (const double*)L.t.p, C.b.p);
        rc = vcycle(mg, l - 1, alpha, beta, C.b.p, C.x.p);
        if (rc) return rc;
        hipLaunchKernelGGL(k_mg_prolongate_add, dim3(grid_for(n, 256)), dim3(256), 0, st, L.N, L.S, (const unsigned*)L.p_off.p,
                           (const unsigned*)L.p_idx.p, (const double*)L.p_w.p, dm, (const double*)C.x.p, x);
        rc = chebyshev(mg, L, alpha, beta, b, x, false);
        if (rc) return rc;
    }
    if (dm) hipLaunchKernelGGL(k_mg_dirichlet_rows, dim3(grid_for(n, 256)), dim3(256), 0, st, n, L.S, dm, b, (const double*)L.diag.p, x);
    HIP_TRY(mg->fine, hipGetLastError());
    return FH_OK;
}

template <class T>
int upload(fh_ctx* f, DevBuf<T>& d, const std::vector<T>& h) {
    HIP_TRY(f, d.alloc(h.size()));
    if (!h.empty()) HIP_TRY(f, hipMemcpy(d.p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
    return FH_OK;
}

int dirichlet_flags(fh_ctx* c, std::vector<unsigned char>& out) {
    out.assign(c->N, 0);
    if (c->mf_num_dirichlet && c->N) {
        HIP_TRY(c, hipMemcpyAsync(out.data(), c->mf_dmask.p, c->N, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return FH_OK;
}
}  // namespace

// ---- used by the solvers (engine_solver.hip): per solve, the injection of u and the cached per-level data; per PCG iteration, one V-cycle
extern "C++" int mg_setup(fh_ctx* fine, double alpha, double beta) {
    fh_mg* mg = fine->mg;
    StreamBorrow borrow(mg);
    const int L = (int)mg->lv.size() - 1;
    int rc = expansion_blocks_multigrid(fine, "FH_PRECOND_MULTIGRID");
    if (rc) return rc;
    // the work vectors, the diagonal and the transfers were sized for each level's mesh at fh_mg_create: a level whose mesh or solution dim has
    // changed since would have S * N entries written into arrays of the old length
    for (int l = 0; l <= L; ++l) {
        const MgLevel& V = mg->lv[l];
        if (V.c->topo_gen != V.topo_gen || (int)V.c->N != V.N || V.c->S() != V.S || !V.c->has_mesh || V.c->ragged)
            return fine->fail(FH_INVALID_STATE, "multigrid level " + std::to_string(l) + ": the level's mesh or operator changed since fh_mg_create (fh_set_mesh*) -- make a new hierarchy");
    }
    for (int l = L - 1; l >= 0; --l) {
        MgLevel& C = mg->lv[l];
        const fh_ctx* src = mg->lv[l + 1].c;
        if (!op_depends_on_u(C.c->op)) continue;
        if (!src->has_u) return fine->fail(FH_INVALID_STATE, "multigrid: a nonlinear coarse level needs u on the level above it");
        hipLaunchKernelGGL(k_mg_inject, dim3(grid_for(C.n, 256)), dim3(256), 0, fine->stream, C.N, C.S, (const unsigned*)mg->lv[l + 1].inj.p,
                           (const double*)src->u.p, C.t.p);
        HIP_TRY(fine, hipGetLastError());
        rc = fh_set_u_dev(C.c, C.t.p);
        if (rc) return fine->fail(rc, std::string("multigrid: setting a coarse level's u: ") + C.c->err);
    }
    for (int l = 0; l <= L; ++l) {
        MgLevel& V = mg->lv[l];
        fh_ctx* c = V.c;
        rc = (alpha == 0.0 && beta == 1.0) ? mf_ready(c, "multigrid", MF_TANGENT) : mf_shift_ready(c, "multigrid", alpha, beta);
        if (rc) return c == fine ? rc : fine->fail(rc, "multigrid level " + std::to_string(l) + ": " + c->err);
        unsigned long long key[8];
        mg_key(c, alpha, beta, key);
        const bool scale_stale = c->mf_num_dirichlet && !std::equal(key, key + 7, c->mf_scale_key);
        if (!V.have_key || scale_stale || !std::equal(key, key + 8, V.key)) {
            V.have_key = false;
            rc = mf_shift_diagonal(c, alpha, beta, V.diag.p, true);
            if (rc) return c == fine ? rc : fine->fail(rc, "multigrid level " + std::to_string(l) + ": " + c->err);
            rc = l == 0 ? factor_coarsest(mg, V, alpha, beta) : estimate_lambda(mg, V, alpha, beta);
            if (rc) return rc;
            std::memcpy(V.key, key, sizeof key);
            V.have_key = true;
        }
        if (c != fine) {
            rc = reset_status(c);
            if (rc) return rc;
        }
    }
    return FH_OK;
}

extern "C++" int mg_precondition(fh_ctx* fine, double alpha, double beta, const double* r, double* z) {
    fh_mg* mg = fine->mg;
    StreamBorrow borrow(mg);
    return vcycle(mg, (int)mg->lv.size() - 1, alpha, beta, r, z);
}

// singular element Jacobians met on the coarse levels during the solve
extern "C++" int mg_finish(fh_ctx* fine) {
    fh_mg* mg = fine->mg;
    StreamBorrow borrow(mg);
    for (size_t l = 0; l + 1 < mg->lv.size(); ++l) {
        const int rc = read_status(mg->lv[l].c, nullptr);
        if (rc) return fine->fail(rc, "multigrid level " + std::to_string(l) + ": " + mg->lv[l].c->err);
    }
    return FH_OK;
}

extern "C++" void mg_orphan(fh_mg* mg) { mg->fine = nullptr; }

extern "C++" void mg_cg_update(hipStream_t st, int blocks, int n, double alpha, const double* p, const double* Ap, double* x, double* r,
                              double* partial) {
    hipLaunchKernelGGL(k_mg_cg_update, dim3(blocks), dim3(256), 0, st, n, alpha, p, Ap, x, r, partial);
}
extern "C++" void mg_cg_zr(hipStream_t st, int blocks, int n, int K, const double* z, const double* r, double* p, double* partial) {
    hipLaunchKernelGGL(k_mg_cg_zr, dim3(blocks), dim3(256), 0, st, n, K, z, r, p, partial);
}

extern "C" {

int fh_mg_create(fh_ctx* fine, uint64_t num_coarse, fh_ctx* const* coarse, const uint64_t* const* transfer_offsets,
                 const uint64_t* const* transfer_indices, const double* const* transfer_weights, fh_mg** out) {
    if (!fine || !out) return FH_BAD_ARGUMENT;
    *out = nullptr;
    DevGuard dev_guard_(fine->device);
    if (num_coarse && (!coarse || !transfer_offsets || !transfer_indices || !transfer_weights))
        return fine->fail(FH_BAD_ARGUMENT, "fh_mg_create: null argument");
    std::vector<fh_ctx*> ctx(coarse, coarse + num_coarse);
    ctx.push_back(fine);
    for (size_t l = 0; l < ctx.size(); ++l) {
        fh_ctx* c = ctx[l];
        if (!c) return fine->fail(FH_BAD_ARGUMENT, "fh_mg_create: null coarse context");
        if (c->device != fine->device) return fine->fail(FH_BAD_ARGUMENT, "fh_mg_create: every level must be on the fine context's device");
        if (!c->has_mesh || c->ragged || c->op < 0) return fine->fail(FH_INVALID_STATE, "fh_mg_create: every level needs a mesh and an operator");
        if (!op_has_stress(c->op)) return fine->fail(FH_UNSUPPORTED, "fh_mg_create: the levels' operators must have a matrix-free map (Laplace, LinearElastic, NeoHookean, StVK, StableNeoHookean)");
        if (c->S() != fine->S()) return fine->fail(FH_BAD_ARGUMENT, "fh_mg_create: the levels differ in solution dim");
        for (size_t k = 0; k < l; ++k)
            if (ctx[k] == c) return fine->fail(FH_BAD_ARGUMENT, "fh_mg_create: a context appears twice");
    }
    const int S = fine->S();
    if ((uint64_t)S * ctx[0]->N > (uint64_t)MG_MAX_COARSE_DOFS)
        return fine->fail(FH_UNSUPPORTED, "fh_mg_create: the coarsest level has more than 4096 dofs");
    auto mg = std::make_unique<fh_mg>();
    mg->fine = fine;
    mg->device = fine->device;
    mg->lv = std::vector<MgLevel>(ctx.size());   // (constructed in place: a level holds device buffers and does not move)
    std::vector<unsigned char> dm_c, dm_f;
    int rc = dirichlet_flags(ctx[0], dm_c);
    if (rc) return fine->fail(rc, ctx[0]->err);
    for (size_t l = 0; l < ctx.size(); ++l) {
        MgLevel& V = mg->lv[l];
        V.c = ctx[l];
        V.S = S;
        V.N = (int)ctx[l]->N;
        V.n = S * V.N;
        V.topo_gen = ctx[l]->topo_gen;
        HIP_TRY(fine, V.diag.alloc(V.n));
        HIP_TRY(fine, V.r.alloc(V.n));
        HIP_TRY(fine, V.d.alloc(V.n));
        HIP_TRY(fine, V.t.alloc(V.n));
        if (l + 1 < ctx.size()) {
            HIP_TRY(fine, V.b.alloc(V.n));
            HIP_TRY(fine, V.x.alloc(V.n));
        }
        if (l == 0) continue;
        // pair l: lv[l - 1] -> lv[l]
        const uint64_t Nf = ctx[l]->N, Nc = ctx[l - 1]->N;
        const uint64_t* off = transfer_offsets[l - 1];
        const uint64_t* idx = transfer_indices[l - 1];
        const double* w = transfer_weights[l - 1];
        if (!off || !idx || !w) return fine->fail(FH_BAD_ARGUMENT, "fh_mg_create: null transfer array");
        if (off[0] != 0) return fine->fail(FH_BAD_ARGUMENT, "fh_mg_create: transfer offsets must start at 0");
        std::vector<unsigned> p_off(Nf + 1), p_idx, inj(Nc, ~0u);
        std::vector<double> p_w;
        std::vector<unsigned> cnt(Nc + 1, 0);
        for (uint64_t i = 0; i < Nf; ++i) {
            if (off[i + 1] < off[i] || off[i + 1] - off[i] > 8 || off[i + 1] == off[i])
                return fine->fail(FH_BAD_ARGUMENT, "fh_mg_create: every transfer row needs 1 to 8 parents");
            p_off[i] = (unsigned)p_idx.size();
            for (uint64_t k = off[i]; k < off[i + 1]; ++k) {
                if (idx[k] >= Nc) return fine->fail(FH_BAD_ARGUMENT, "fh_mg_create: transfer index out of range");
                p_idx.push_back((unsigned)idx[k]);
                p_w.push_back(w[k]);
                ++cnt[idx[k] + 1];
            }
            if (off[i + 1] - off[i] == 1 && w[off[i]] == 1.0) {
                if (inj[idx[off[i]]] != ~0u) return fine->fail(FH_BAD_ARGUMENT, "fh_mg_create: a coarse node is injected into two fine nodes");
                inj[idx[off[i]]] = (unsigned)i;
            }
        }
        p_off[Nf] = (unsigned)p_idx.size();
        for (uint64_t j = 0; j < Nc; ++j)
            if (inj[j] == ~0u) return fine->fail(FH_BAD_ARGUMENT, "fh_mg_create: a coarse node has no injected fine copy (a row with one parent of weight 1)");
        rc = dirichlet_flags(ctx[l], dm_f);
        if (rc) return fine->fail(rc, ctx[l]->err);
        const unsigned comps = (1u << ctx[l]->S()) - 1u;   // (a node set holds all ones: only the components of the solution count)
        for (uint64_t j = 0; j < Nc; ++j)
            if ((dm_c[j] & comps) != (dm_f[inj[j]] & comps))
                return fine->fail(FH_BAD_ARGUMENT, "fh_mg_create: a coarse node must constrain exactly the components its injected fine node does (coarse node " +
                                                       std::to_string(j) + " of level " + std::to_string(l - 1) + ")");
        // the transpose, rows in ascending fine index
        for (uint64_t j = 0; j < Nc; ++j) cnt[j + 1] += cnt[j];
        std::vector<unsigned> r_off(cnt.begin(), cnt.end()), r_idx(p_idx.size()), fill(cnt.begin(), cnt.end() - 1);
        std::vector<double> r_w(p_idx.size());
        for (uint64_t i = 0; i < Nf; ++i)
            for (unsigned k = p_off[i]; k < p_off[i + 1]; ++k) {
                const unsigned pos = fill[p_idx[k]]++;
                r_idx[pos] = (unsigned)i;
                r_w[pos] = p_w[k];
            }
        if ((rc = upload(fine, V.p_off, p_off)) || (rc = upload(fine, V.p_idx, p_idx)) || (rc = upload(fine, V.p_w, p_w)) ||
            (rc = upload(fine, V.r_off, r_off)) || (rc = upload(fine, V.r_idx, r_idx)) || (rc = upload(fine, V.r_w, r_w)) ||
            (rc = upload(fine, V.inj, inj)))
            return rc;
        dm_c.swap(dm_f);
    }
    *out = mg.release();
    return FH_OK;
}

// touches no coarse context, and the fine one only while it is alive (fh_destroy of a fine context clears mg->fine)
void fh_mg_destroy(fh_mg* mg) {
    if (!mg) return;
    DevGuard dev_guard_(mg->device);
    if (mg->fine && mg->fine->mg == mg) {
        (void)hipStreamSynchronize(mg->fine->stream);
        mg->fine->mg = nullptr;
    }
    delete mg;
}

int fh_set_multigrid(fh_ctx* fine, fh_mg* mg) {
    if (!fine) return FH_BAD_ARGUMENT;
    if (mg && mg->fine != fine) return fine->fail(FH_BAD_ARGUMENT, "fh_set_multigrid: the hierarchy was made for another fine context");
    if (fine->mg && fine->mg != mg) mg_orphan(fine->mg);   // the one it replaces is orphaned: fh_mg_destroy will not touch this context
    fine->mg = mg;
    return FH_OK;
}

int fh_mg_set_smoother(fh_mg* mg, uint32_t degree, double range, uint32_t eig_steps) {
    if (!mg || !mg->fine) return FH_BAD_ARGUMENT;
    if (degree < 1 || degree > 64 || !(range > 1.0) || eig_steps < 1 || eig_steps > 200)
        return mg->fine->fail(FH_BAD_ARGUMENT, "fh_mg_set_smoother: degree 1..64, range > 1, eig_steps 1..200");
    mg->degree = degree;
    mg->range = range;
    mg->eig_steps = eig_steps;
    for (auto& l : mg->lv) l.have_key = false;
    return FH_OK;
}

int fh_mg_level_info(fh_mg* mg, uint32_t level, double* lambda_max, uint64_t* num_dofs) {
    if (!mg || !mg->fine) return FH_BAD_ARGUMENT;
    if (level >= mg->lv.size()) return mg->fine->fail(FH_BAD_ARGUMENT, "fh_mg_level_info: no such level");
    if (lambda_max) *lambda_max = mg->lv[level].lambda;
    if (num_dofs) *num_dofs = (uint64_t)mg->lv[level].n;
    return FH_OK;
}

int fh_mg_apply_dev(fh_mg* mg, double alpha, double beta, const double* r_dev, double* z_dev) {
    if (!mg || !mg->fine) return FH_BAD_ARGUMENT;
    fh_ctx* f = mg->fine;
    DevGuard dev_guard_(f->device);
    if (!r_dev || !z_dev || r_dev == z_dev) return f->fail(FH_BAD_ARGUMENT, "fh_mg_apply_dev: null or aliased vectors");
    if (f->mg != mg) return f->fail(FH_INVALID_STATE, "fh_mg_apply_dev: attach the hierarchy with fh_set_multigrid first");
    if (contact_table(f).count)
        return f->fail(FH_UNSUPPORTED, "fh_mg_apply_dev: obstacles are set (fh_set_obstacles): the coarse levels would not see the contact term");
    int rc = mg_setup(f, alpha, beta);
    if (rc) return rc;
    rc = reset_status(f);
    if (rc) return rc;
    rc = mg_precondition(f, alpha, beta, r_dev, z_dev);
    if (rc) return rc;
    rc = read_status(f, nullptr);
    if (rc) return rc;
    rc = mg_finish(f);
    if (rc) return rc;
    HIP_TRY(f, hipStreamSynchronize(f->stream));
    return FH_OK;
}

}  // extern "C"
