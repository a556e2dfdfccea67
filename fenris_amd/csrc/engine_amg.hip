// Smoothed-aggregation algebraic multigrid on the assembled matrix (fh_amg): FH_PRECOND_AMG of fh_cg_solve(_dev) and fh_amg_apply_dev.
//
// Levels: lv[0] is the fine level (the context's pattern and the caller's values, borrowed), lv[L] the coarsest.  Level l < L owns its
// aggregates, T, P (block rows: its nodes), P^T (block rows: the aggregates), the product A P and, through lv[l + 1], A_c = P^T (A P).
// Setup splits into a symbolic part (aggregation, T, every pattern: create only) and a numeric part (the diagonal, lambda, the values of
// P, P^T, A P, A_c, and the coarse factor: create and fh_amg_update_values), which run the same kernels in the same order, so a refresh
// gives the bits of a create with the same aggregates.  All work runs on the context's stream; the V-cycle reuses the Chebyshev,
// eigenvalue-estimate and dense-inverse code of engine_mg.hip.
#include <memory>

#include "amg_kernels.hpp"
#include "engine_internal.hpp"
#include "mg_kernels.hpp"

using namespace fenris_hip_amg;
using namespace fenris_hip_mg;

namespace {
constexpr int AMG_MAX_COARSE_DOFS = 4096;

struct AmgLevel {
    int N = 0, R = 0, n = 0, C = 0;   // nodes, block size, dofs; C: the block size of the next level (nb)
    const unsigned *off = nullptr, *cols = nullptr;
    const double* vals = nullptr;
    uint64_t nnz = 0;                  // blocks of A
    DevBuf<unsigned> own_off, own_cols, a_row;
    DevBuf<double> own_vals;
    DevBuf<double> diag, dnorm, B, b, x, r, d, t, iso_inv;
    DevBuf<unsigned char> iso;
    bool any_iso = false;
    double lambda = 0.0;
    // transfer to the next level
    int nagg = 0;
    DevBuf<unsigned> agg, p_off, p_cols, p_row, pt_off, pt_cols, pt_row, pt_src, ap_off, ap_cols, ap_row;
    DevBuf<double> T, p_vals, pt_vals, ap_vals;
    uint64_t nnz_p = 0, nnz_ap = 0;
};
}  // namespace

struct fh_amg {
    fh_ctx* c = nullptr;   // null once the context was destroyed (fh_destroy orphans an attached hierarchy)
    int device = 0;
    std::vector<std::unique_ptr<AmgLevel>> lv;
    uint32_t degree = 3, eig_steps = 10;
    double range = 15.0;
    DevBuf<double> ainv;   // coarsest level: the dense inverse, row-major
    // level 0 holds the context's noff / ncols pointers, N and nnz: the pattern build and the solution dim they were read at
    unsigned long long pattern_gen = 0;
    int S = 0;
};

namespace {
int G(long long n) { return grid_for(n, 256, 1 << 20); }

int spmv(fh_amg* h, AmgLevel& L, int which, const double* x, double* y, bool accumulate) {
    fh_ctx* c = h->c;
    hipStream_t st = c->stream;
    // which 0: A (R x R blocks), 1: P (R x C), 2: P^T (C x R)
    if (which == 0 && L.vals == nullptr) return FH_OK;
    const unsigned *off, *cols;
    const double* v;
    int rows, R, Cb;
    if (which == 0) { off = L.off; cols = L.cols; v = L.vals; rows = L.n; R = L.R; Cb = L.R; }
    else if (which == 1) { off = L.p_off.p; cols = L.p_cols.p; v = L.p_vals.p; rows = L.n; R = L.R; Cb = L.C; }
    else { off = L.pt_off.p; cols = L.pt_cols.p; v = L.pt_vals.p; rows = L.nagg * L.C; R = L.C; Cb = L.R; }
    if (rows == 0) return FH_OK;
    const int g = G(rows);
    dispatch_or_last(int_list<1, 2, 3, 4, 5, 6>{}, Cb, [&](auto cb) {   // (columns per block: anything else runs as 6)
        hipLaunchKernelGGL(k_amg_spmv<cb()>, dim3(g), dim3(256), 0, st, rows, R, off, cols, v, x, y, (int)accumulate);
        return 0;
    });
    HIP_TRY(c, hipGetLastError());
    return FH_OK;
}

// y = A x on level l: the fine level through the assembled SpMV of the context, the coarse ones through k_amg_spmv
int apply_a(fh_amg* h, int l, const double* x, double* y, DevBuf<double>* dots, int* count) {
    AmgLevel& L = *h->lv[l];
    fh_ctx* c = h->c;
    const int rc = l == 0 ? csr_spmv(c, L.vals, x, y) : spmv(h, L, 0, x, y, false);
    if (rc) return rc;
    if (dots) {
        const int g = std::min(1024, std::max(1, (L.n + 255) / 256));
        if (dots->n < (size_t)g) HIP_TRY(c, dots->alloc(g));
        hipLaunchKernelGGL(k_amg_dot_partials, dim3(g), dim3(256), 0, c->stream, L.n, x, y, dots->p);
        HIP_TRY(c, hipGetLastError());
        *count = g;
    }
    return FH_OK;
}

template <class T>
int zeros(fh_ctx* c, DevBuf<T>& d, size_t n) {
    HIP_TRY(c, d.alloc(n));
    HIP_TRY(c, hipMemsetAsync(d.p, 0, sizeof(T) * std::max<size_t>(n, 1), c->stream));
    return FH_OK;
}

int scan(fh_ctx* c, unsigned* in_out, int n_plus_1) {   // exclusive sum in place
    size_t bytes = 0;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, in_out, in_out, n_plus_1, c->stream));
    DevBuf<unsigned char> tmp;
    HIP_TRY(c, tmp.alloc(bytes));
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(tmp.p, bytes, in_out, in_out, n_plus_1, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // (tmp is released on return)
    return FH_OK;
}

unsigned read_u32(fh_ctx* c, const unsigned* p, int* rc) {
    unsigned v = 0;
    *rc = FH_OK;
    if (hipMemcpyAsync(&v, p, sizeof v, hipMemcpyDeviceToHost, c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
        *rc = c->fail(FH_HIP_ERROR, "amg: reading a count");
    return v;
}

// stable counting sort of the m items by key into seg_off (K + 1) and item
int counting_sort(fh_ctx* c, long long m, const unsigned* key, int K, DevBuf<unsigned>& seg_off, DevBuf<unsigned>& item) {
    int rc = zeros(c, seg_off, (size_t)K + 1);
    if (rc) return rc;
    DevBuf<unsigned> cursor;
    if ((rc = zeros(c, cursor, (size_t)K + 1))) return rc;
    if (m) hipLaunchKernelGGL(k_amg_count_keys, dim3(G(m)), dim3(256), 0, c->stream, m, key, seg_off.p);
    HIP_TRY(c, hipGetLastError());
    if ((rc = scan(c, seg_off.p, K + 1))) return rc;
    const unsigned total = read_u32(c, seg_off.p + K, &rc);
    if (rc) return rc;
    HIP_TRY(c, item.alloc(total));
    if (m) hipLaunchKernelGGL(k_amg_place, dim3(G(m)), dim3(256), 0, c->stream, m, key, seg_off.p, cursor.p, item.p);
    if (K) hipLaunchKernelGGL(k_amg_sort_segments, dim3(G(K)), dim3(256), 0, c->stream, K, seg_off.p, item.p);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FH_OK;
}

// the pattern of X Y (rows N) into z_off, z_cols, z_row
int spgemm_pattern(fh_ctx* c, int N, const unsigned* x_off, const unsigned* x_cols, const unsigned* y_off, const unsigned* y_cols, DevBuf<unsigned>& z_off,
                   DevBuf<unsigned>& z_cols, DevBuf<unsigned>& z_row, uint64_t* nnz) {
    int rc = zeros(c, z_off, (size_t)N + 1);
    if (rc) return rc;
    DevBuf<int> over;
    if ((rc = zeros(c, over, 1))) return rc;
    if (N) hipLaunchKernelGGL(k_amg_spgemm_pattern, dim3(G(N)), dim3(256), 0, c->stream, N, x_off, x_cols, y_off, y_cols, z_off.p, (const unsigned*)nullptr,
                              (unsigned*)nullptr, over.p);
    HIP_TRY(c, hipGetLastError());
    int h_over = 0;
    HIP_TRY(c, hipMemcpyAsync(&h_over, over.p, sizeof h_over, hipMemcpyDeviceToHost, c->stream));
    if ((rc = scan(c, z_off.p, N + 1))) return rc;
    if (h_over) return c->fail(FH_UNSUPPORTED, "fh_amg_create: a row of a Galerkin product has more than 512 blocks");
    *nnz = read_u32(c, z_off.p + N, &rc);
    if (rc) return rc;
    HIP_TRY(c, z_cols.alloc(*nnz));
    HIP_TRY(c, z_row.alloc(*nnz));
    if (N) {
        hipLaunchKernelGGL(k_amg_spgemm_pattern, dim3(G(N)), dim3(256), 0, c->stream, N, x_off, x_cols, y_off, y_cols, (unsigned*)nullptr,
                           (const unsigned*)z_off.p, z_cols.p, over.p);
        hipLaunchKernelGGL(k_amg_fill_rows, dim3(G(N)), dim3(256), 0, c->stream, N, (const unsigned*)z_off.p, z_row.p);
    }
    HIP_TRY(c, hipGetLastError());
    return FH_OK;
}

// ---- symbolic coarsening of level l: strength, aggregates, T and the coarse B, the patterns of P, P^T, A P and A_c (into lv[l + 1])
int coarsen_symbolic(fh_amg* h, int l, double theta) {
    fh_ctx* c = h->c;
    hipStream_t st = c->stream;
    AmgLevel& L = *h->lv[l];
    const int N = L.N;
    int rc;
    DevBuf<unsigned char> strong, state;
    HIP_TRY(c, strong.alloc(L.nnz));
    HIP_TRY(c, state.alloc(N));
    hipLaunchKernelGGL(k_amg_strength, dim3(G(N)), dim3(256), 0, st, N, L.R, L.off, L.cols, L.vals, (const double*)L.dnorm.p, theta, strong.p, L.iso.p);
    DevBuf<int> flag;
    if ((rc = zeros(c, flag, 1))) return rc;
    hipLaunchKernelGGL(k_amg_state_init, dim3(G(N)), dim3(256), 0, st, N, (const unsigned char*)L.iso.p, state.p, flag.p);
    HIP_TRY(c, hipGetLastError());
    {
        int any = 0;
        HIP_TRY(c, hipMemcpyAsync(&any, flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        L.any_iso = any != 0;
    }
    // distance-2 MIS in synchronous rounds
    DevBuf<unsigned long long> v0, v1;
    HIP_TRY(c, v0.alloc(N));
    HIP_TRY(c, v1.alloc(N));
    for (int round = 0;; ++round) {
        if (round > N + 1) return c->fail(FH_HIP_ERROR, "fh_amg_create: the independent set did not converge");
        HIP_TRY(c, hipMemsetAsync(flag.p, 0, sizeof(int), st));
        hipLaunchKernelGGL(k_amg_mis_value, dim3(G(N)), dim3(256), 0, st, N, (const unsigned char*)state.p, v0.p);
        hipLaunchKernelGGL(k_amg_mis_max, dim3(G(N)), dim3(256), 0, st, N, L.off, L.cols, (const unsigned char*)strong.p, (const unsigned long long*)v0.p, v1.p);
        hipLaunchKernelGGL(k_amg_mis_max, dim3(G(N)), dim3(256), 0, st, N, L.off, L.cols, (const unsigned char*)strong.p, (const unsigned long long*)v1.p, v0.p);
        hipLaunchKernelGGL(k_amg_mis_update, dim3(G(N)), dim3(256), 0, st, N, state.p, (const unsigned long long*)v0.p, flag.p);
        HIP_TRY(c, hipGetLastError());
        int undecided = 0;
        HIP_TRY(c, hipMemcpyAsync(&undecided, flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        if (!undecided) break;
    }
    DevBuf<unsigned> rank, agg0;
    HIP_TRY(c, rank.alloc((size_t)N + 1));
    HIP_TRY(c, agg0.alloc(N));
    HIP_TRY(c, L.agg.alloc(N));
    hipLaunchKernelGGL(k_amg_root_flags, dim3(G(N + 1)), dim3(256), 0, st, N, (const unsigned char*)state.p, rank.p);
    HIP_TRY(c, hipGetLastError());
    if ((rc = scan(c, rank.p, N + 1))) return rc;
    L.nagg = (int)read_u32(c, rank.p + N, &rc);
    if (rc) return rc;
    HIP_TRY(c, hipMemsetAsync(flag.p, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_amg_join, dim3(G(N)), dim3(256), 0, st, N, L.off, L.cols, (const unsigned char*)strong.p, (const unsigned char*)state.p,
                       (const unsigned*)rank.p, agg0.p);
    hipLaunchKernelGGL(k_amg_sweep, dim3(G(N)), dim3(256), 0, st, N, L.off, L.cols, (const unsigned char*)strong.p, (const unsigned char*)state.p,
                       (const unsigned*)agg0.p, L.agg.p, flag.p);
    HIP_TRY(c, hipGetLastError());
    int left = 0;
    HIP_TRY(c, hipMemcpyAsync(&left, flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (left) return c->fail(FH_HIP_ERROR, "fh_amg_create: a node was left without an aggregate");
    if (L.nagg == 0) return c->fail(FH_UNSUPPORTED, "fh_amg_create: every node of a level above 4096 dofs is isolated");
    if ((double)L.nagg * L.C > 0.9 * L.n)
        return c->fail(FH_UNSUPPORTED, "fh_amg_create: a coarsening step keeps more than 90 % of the dofs (level " + std::to_string(l) + ")");
    // T and the coarse near-nullspace
    auto next = std::make_unique<AmgLevel>();
    AmgLevel& Cn = *next;
    Cn.N = L.nagg;
    Cn.R = L.C;
    Cn.C = L.C;
    Cn.n = Cn.N * Cn.R;
    {
        DevBuf<unsigned> agg_off, members;
        if ((rc = counting_sort(c, N, L.agg.p, L.nagg, agg_off, members))) return rc;
        if ((rc = zeros(c, L.T, (size_t)L.n * L.C))) return rc;
        HIP_TRY(c, Cn.B.alloc((size_t)Cn.n * Cn.C));
        hipLaunchKernelGGL(k_amg_tentative, dim3(grid_for(L.nagg, 64, 1 << 20)), dim3(64), 0, st, L.nagg, L.R, L.C, (const unsigned*)agg_off.p,
                           (const unsigned*)members.p, (const double*)L.B.p, L.T.p, Cn.B.p);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipStreamSynchronize(st));
    }
    // P's pattern
    if ((rc = zeros(c, L.p_off, (size_t)N + 1))) return rc;
    hipLaunchKernelGGL(k_amg_p_pattern, dim3(G(N)), dim3(256), 0, st, N, L.off, L.cols, (const unsigned*)L.agg.p, L.p_off.p, (const unsigned*)nullptr,
                       (unsigned*)nullptr);
    HIP_TRY(c, hipGetLastError());
    if ((rc = scan(c, L.p_off.p, N + 1))) return rc;
    L.nnz_p = read_u32(c, L.p_off.p + N, &rc);
    if (rc) return rc;
    HIP_TRY(c, L.p_cols.alloc(L.nnz_p));
    HIP_TRY(c, L.p_row.alloc(L.nnz_p));
    HIP_TRY(c, L.p_vals.alloc(L.nnz_p * L.R * L.C));
    hipLaunchKernelGGL(k_amg_p_pattern, dim3(G(N)), dim3(256), 0, st, N, L.off, L.cols, (const unsigned*)L.agg.p, (unsigned*)nullptr,
                       (const unsigned*)L.p_off.p, L.p_cols.p);
    hipLaunchKernelGGL(k_amg_fill_rows, dim3(G(N)), dim3(256), 0, st, N, (const unsigned*)L.p_off.p, L.p_row.p);
    HIP_TRY(c, hipGetLastError());
    // P^T: P's entries sorted by column, stably (ascending fine node)
    if ((rc = counting_sort(c, (long long)L.nnz_p, L.p_cols.p, L.nagg, L.pt_off, L.pt_src))) return rc;
    HIP_TRY(c, L.pt_cols.alloc(L.nnz_p));
    HIP_TRY(c, L.pt_row.alloc(L.nnz_p));
    HIP_TRY(c, L.pt_vals.alloc(L.nnz_p * L.R * L.C));
    hipLaunchKernelGGL(k_amg_fill_rows, dim3(G(L.nagg)), dim3(256), 0, st, L.nagg, (const unsigned*)L.pt_off.p, L.pt_row.p);
    if (L.nnz_p)
        hipLaunchKernelGGL(k_amg_gather, dim3(G((long long)L.nnz_p)), dim3(256), 0, st, (long long)L.nnz_p, (const unsigned*)L.pt_src.p,
                           (const unsigned*)L.p_row.p, L.pt_cols.p);
    HIP_TRY(c, hipGetLastError());
    // A P and A_c = P^T (A P)
    if ((rc = spgemm_pattern(c, N, L.off, L.cols, L.p_off.p, L.p_cols.p, L.ap_off, L.ap_cols, L.ap_row, &L.nnz_ap))) return rc;
    HIP_TRY(c, L.ap_vals.alloc(L.nnz_ap * L.R * L.C));
    if ((rc = spgemm_pattern(c, L.nagg, L.pt_off.p, L.pt_cols.p, L.ap_off.p, L.ap_cols.p, Cn.own_off, Cn.own_cols, Cn.a_row, &Cn.nnz))) return rc;
    HIP_TRY(c, Cn.own_vals.alloc(Cn.nnz * Cn.R * Cn.R));
    Cn.off = Cn.own_off.p;
    Cn.cols = Cn.own_cols.p;
    Cn.vals = Cn.own_vals.p;
    HIP_TRY(c, hipStreamSynchronize(st));
    h->lv.push_back(std::move(next));
    return FH_OK;
}
}  // namespace

namespace {
// the point diagonal (zero: +inf) and the block norms of level l
int level_diag(fh_amg* h, int l) {
    fh_ctx* c = h->c;
    AmgLevel& L = *h->lv[l];
    if (L.diag.n < (size_t)L.n || L.n == 0) {
        HIP_TRY(c, L.diag.alloc(L.n));
        HIP_TRY(c, L.dnorm.alloc(L.N));
    }
    if (L.N) hipLaunchKernelGGL(k_amg_diag, dim3(G(L.N)), dim3(256), 0, c->stream, L.N, L.R, L.off, L.cols, L.vals, L.dnorm.p, L.diag.p);
    HIP_TRY(c, hipGetLastError());
    return FH_OK;
}

// lambda, P = (I - omega D^-1 A) T, P^T, A P and A_c = P^T (A P) of level l (its patterns made by coarsen_symbolic)
int numeric_transfer(fh_amg* h, int l) {
    fh_ctx* c = h->c;
    hipStream_t st = c->stream;
    AmgLevel& L = *h->lv[l];
    AmgLevel& Cn = *h->lv[l + 1];
    if (L.any_iso) {
        if (L.iso_inv.n < (size_t)L.N * L.R * L.R) HIP_TRY(c, L.iso_inv.alloc((size_t)L.N * L.R * L.R));
        hipLaunchKernelGGL(k_amg_iso_inverse, dim3(grid_for(L.N, 64, 1 << 20)), dim3(64), 0, st, L.N, L.R, L.off, L.cols, L.vals,
                           (const unsigned char*)L.iso.p, L.iso_inv.p);
        HIP_TRY(c, hipGetLastError());
    }
    int rc = mg_estimate_lambda(c, st, L.n, L.R, L.any_iso ? L.iso.p : nullptr, L.diag.p, h->eig_steps,
                                [&](const double* x, double* y, DevBuf<double>* dots, int* count) { return apply_a(h, l, x, y, dots, count); }, "amg",
                                &L.lambda);
    if (rc) return rc;
    const double omega = 4.0 / (3.0 * L.lambda);
    if (L.nnz_p) {
        hipLaunchKernelGGL(k_amg_p_values, dim3(G((long long)L.nnz_p)), dim3(256), 0, st, (long long)L.nnz_p, L.R, L.C, (const unsigned*)L.p_row.p,
                           (const unsigned*)L.p_off.p, (const unsigned*)L.p_cols.p, L.off, L.cols, L.vals, (const unsigned*)L.agg.p,
                           (const double*)L.T.p, (const double*)L.diag.p, omega, L.p_vals.p);
        hipLaunchKernelGGL(k_amg_transpose_values, dim3(G((long long)L.nnz_p)), dim3(256), 0, st, (long long)L.nnz_p, L.R, L.C,
                           (const unsigned*)L.pt_row.p, (const unsigned*)L.pt_off.p, (const unsigned*)L.pt_src.p, (const unsigned*)L.p_row.p,
                           (const unsigned*)L.p_off.p, (const double*)L.p_vals.p, L.pt_vals.p);
    }
    if (L.nnz_ap)
        hipLaunchKernelGGL(k_amg_spgemm_values, dim3(G((long long)L.nnz_ap)), dim3(256), 0, st, (long long)L.nnz_ap, L.R, L.R, L.C,
                           (const unsigned*)L.ap_row.p, (const unsigned*)L.ap_off.p, (const unsigned*)L.ap_cols.p, L.off, L.cols, L.vals,
                           (const unsigned*)L.p_off.p, (const unsigned*)L.p_cols.p, (const double*)L.p_vals.p, L.ap_vals.p, 0);
    if (Cn.nnz) {
        hipLaunchKernelGGL(k_amg_spgemm_values, dim3(G((long long)Cn.nnz)), dim3(256), 0, st, (long long)Cn.nnz, L.C, L.R, L.C,
                           (const unsigned*)Cn.a_row.p, Cn.off, Cn.cols, (const unsigned*)L.pt_off.p, (const unsigned*)L.pt_cols.p,
                           (const double*)L.pt_vals.p, (const unsigned*)L.ap_off.p, (const unsigned*)L.ap_cols.p, (const double*)L.ap_vals.p,
                           Cn.own_vals.p, 1);
        hipLaunchKernelGGL(k_amg_mirror, dim3(G((long long)Cn.nnz)), dim3(256), 0, st, (long long)Cn.nnz, L.C, (const unsigned*)Cn.a_row.p, Cn.off,
                           Cn.cols, Cn.own_vals.p);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(st));
    return FH_OK;
}

// the coarsest level's dense inverse: its matrix downloaded, dofs with a zero diagonal left out (their rows of the inverse are zero)
int factor_coarsest(fh_amg* h) {
    fh_ctx* c = h->c;
    AmgLevel& L = *h->lv.back();
    const int n = L.n, R = L.R, N = L.N;
    if (n == 0) return FH_OK;
    std::vector<unsigned> off(N + 1), cols;
    HIP_TRY(c, hipMemcpyAsync(off.data(), L.off, sizeof(unsigned) * (N + 1), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    cols.resize(off[N]);
    std::vector<double> v((size_t)off[N] * R * R);
    if (off[N]) {
        HIP_TRY(c, hipMemcpyAsync(cols.data(), L.cols, sizeof(unsigned) * cols.size(), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(v.data(), L.vals, sizeof(double) * v.size(), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::vector<double> A((size_t)n * n, 0.0);
    for (int i = 0; i < N; ++i) {
        const unsigned cnt = off[i + 1] - off[i];
        for (int a = 0; a < R; ++a)
            for (unsigned kk = 0; kk < cnt; ++kk)
                for (int b = 0; b < R; ++b)
                    A[(size_t)(R * i + a) * n + (size_t)R * cols[off[i] + kk] + b] = v[(size_t)R * R * off[i] + (size_t)a * R * cnt + (size_t)R * kk + b];
    }
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            const double m = 0.5 * (A[(size_t)i * n + j] + A[(size_t)j * n + i]);
            A[(size_t)i * n + j] = A[(size_t)j * n + i] = m;
        }
    std::vector<char> off_dof(n, 0);
    for (int i = 0; i < n; ++i)
        if (A[(size_t)i * n + i] == 0.0) {
            off_dof[i] = 1;
            for (int j = 0; j < n; ++j) A[(size_t)i * n + j] = A[(size_t)j * n + i] = 0.0;
            A[(size_t)i * n + i] = 1.0;
        }
    std::vector<double> Ainv;
    int rc = mg_dense_inverse(c, "amg", A, n, Ainv, 1e-12);   // (semidefinite coarsest levels: free-floating bodies)
    if (rc) return rc;
    for (int i = 0; i < n; ++i)
        if (off_dof[i])
            for (int j = 0; j < n; ++j) Ainv[(size_t)i * n + j] = Ainv[(size_t)j * n + i] = 0.0;
    if (h->ainv.n < (size_t)n * n) HIP_TRY(c, h->ainv.alloc((size_t)n * n));
    HIP_TRY(c, hipMemcpyAsync(h->ainv.p, Ainv.data(), sizeof(double) * Ainv.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FH_OK;
}

// every numeric quantity, level by level: what a refresh does, and what a create does after each level's symbolic step
int numeric_all(fh_amg* h) {
    const int last = (int)h->lv.size() - 1;
    int rc;
    for (int l = 0; l < last; ++l)
        if ((rc = level_diag(h, l)) || (rc = numeric_transfer(h, l))) return rc;
    if ((rc = level_diag(h, last))) return rc;
    return factor_coarsest(h);
}

int vcycle(fh_amg* h, int l, const double* b, double* x) {
    fh_ctx* c = h->c;
    hipStream_t st = c->stream;
    AmgLevel& L = *h->lv[l];
    const int n = L.n;
    if (n == 0) return FH_OK;
    int rc;
    if (l + 1 == (int)h->lv.size()) {
        hipLaunchKernelGGL(k_mg_dense_apply, dim3((n + 3) / 4), dim3(256), 0, st, n, (const double*)h->ainv.p, b, x);
        HIP_TRY(c, hipGetLastError());
        return FH_OK;
    }
    AmgLevel& Cn = *h->lv[l + 1];
    const LevelApply apply = [&](const double* in, double* out, DevBuf<double>* dots, int* count) { return apply_a(h, l, in, out, dots, count); };
    rc = mg_chebyshev(st, apply, n, L.diag.p, L.lambda, h->degree, h->range, L.r.p, L.d.p, L.t.p, b, x, true);
    if (rc) return rc;
    if ((rc = apply_a(h, l, x, L.t.p, nullptr, nullptr))) return rc;
    hipLaunchKernelGGL(k_amg_residual, dim3(G(n)), dim3(256), 0, st, n, b, (const double*)L.t.p, L.d.p);
    if ((rc = spmv(h, L, 2, L.d.p, Cn.b.p, false))) return rc;
    if ((rc = vcycle(h, l + 1, Cn.b.p, Cn.x.p))) return rc;
    if ((rc = spmv(h, L, 1, Cn.x.p, x, true))) return rc;
    rc = mg_chebyshev(st, apply, n, L.diag.p, L.lambda, h->degree, h->range, L.r.p, L.d.p, L.t.p, b, x, false);
    if (rc) return rc;
    if (L.any_iso)
        hipLaunchKernelGGL(k_amg_iso_apply, dim3(G(n)), dim3(256), 0, st, L.N, L.R, (const unsigned char*)L.iso.p, (const double*)L.iso_inv.p, b, x);
    HIP_TRY(c, hipGetLastError());
    return FH_OK;
}

int level_vectors(fh_ctx* c, AmgLevel& L) {
    HIP_TRY(c, L.b.alloc(L.n));
    HIP_TRY(c, L.x.alloc(L.n));
    HIP_TRY(c, L.r.alloc(L.n));
    HIP_TRY(c, L.d.alloc(L.n));
    HIP_TRY(c, L.t.alloc(L.n));
    HIP_TRY(c, L.iso.alloc(L.N));
    HIP_TRY(c, hipMemsetAsync(L.iso.p, 0, std::max(1, L.N), c->stream));
    return FH_OK;
}

int near_nullspace(fh_ctx* c, AmgLevel& L, int kind, const double* B) {
    hipStream_t st = c->stream;
    HIP_TRY(c, L.B.alloc((size_t)L.n * L.C));
    if (L.N == 0) return FH_OK;
    if (kind == FH_AMG_USER) {
        HIP_TRY(c, hipMemcpyAsync(L.B.p, B, sizeof(double) * L.n * L.C, hipMemcpyHostToDevice, st));
    } else if (kind == FH_AMG_CONSTANT) {
        hipLaunchKernelGGL(k_amg_constant, dim3(G(L.N)), dim3(256), 0, st, L.N, L.R, L.B.p);
    } else {
        const int d = c->ei.d, g = std::min(1024, (L.N + 255) / 256);
        DevBuf<double> partial;
        HIP_TRY(c, partial.alloc((size_t)3 * g));
        hipLaunchKernelGGL(k_amg_coord_partials, dim3(g), dim3(256), 0, st, L.N, d, (const double*)c->verts.p, partial.p);
        HIP_TRY(c, hipGetLastError());
        double s[3];
        const int rc = sum_partials(c, partial.p, g, 3, s);
        if (rc) return rc;
        hipLaunchKernelGGL(k_amg_rigid_body, dim3(G(L.N)), dim3(256), 0, st, L.N, d, (const double*)c->verts.p, s[0] / L.N, s[1] / L.N, s[2] / L.N, L.B.p);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(st));
    return FH_OK;
}
}  // namespace

extern "C++" int amg_precondition(fh_amg* h, const double* r, double* z) { return vcycle(h, 0, r, z); }
// a pattern rebuilt since (fh_set_mesh*, fh_set_connectivity_ragged, then fh_pattern) frees or resizes what level 0 points into; another
// solution dim (fh_set_operator) changes the block size under the same node-level arrays
extern "C++" int amg_current(fh_amg* h, const char* who) {
    fh_ctx* c = h->c;
    if (c->has_pattern && c->pattern_gen == h->pattern_gen && c->S() == h->S) return FH_OK;
    return c->fail(FH_INVALID_STATE, std::string(who) + ": the context's pattern changed since fh_amg_create (fh_set_mesh*, fh_pattern or fh_set_operator) -- make a new hierarchy");
}
extern "C++" void amg_orphan(fh_amg* h) { h->c = nullptr; }

extern "C" {

int fh_amg_create(fh_ctx* c, const double* values_dev, int nullspace, const double* B, uint32_t nb, double theta, uint32_t max_levels, fh_amg** out) {
    if (!c || !out) return FH_BAD_ARGUMENT;
    *out = nullptr;
    DevGuard dev_guard_(c->device);
    if (!c->has_pattern) return c->fail(FH_INVALID_STATE, "fh_amg_create: call fh_pattern first");
    const int S = c->S();
    if (S < 1 || S > 3) return c->fail(FH_UNSUPPORTED, "fh_amg_create: solution dim must be 1..3");
    if (!values_dev) return c->fail(FH_BAD_ARGUMENT, "fh_amg_create: null values");
    if (!(theta >= 0.0)) return c->fail(FH_BAD_ARGUMENT, "fh_amg_create: theta must be >= 0");
    int C;
    if (nullspace == FH_AMG_CONSTANT) {
        C = S;
    } else if (nullspace == FH_AMG_RIGID_BODY) {
        if (!c->has_mesh || c->ragged || S != c->ei.d) return c->fail(FH_BAD_ARGUMENT, "fh_amg_create: rigid-body modes need a mesh and solution dim = d");
        C = c->ei.d == 2 ? 3 : 6;
    } else if (nullspace == FH_AMG_USER) {
        if (!B) return c->fail(FH_BAD_ARGUMENT, "fh_amg_create: FH_AMG_USER needs B");
        if (nb < 1 || nb > 6) return c->fail(FH_BAD_ARGUMENT, "fh_amg_create: nb must be 1..6");
        C = (int)nb;
    } else {
        return c->fail(FH_BAD_ARGUMENT, "fh_amg_create: unknown near-nullspace kind");
    }
    if (max_levels == 0) max_levels = 10;
    auto h = std::make_unique<fh_amg>();
    h->c = c;
    h->device = c->device;
    h->pattern_gen = c->pattern_gen;
    h->S = S;
    auto l0 = std::make_unique<AmgLevel>();
    l0->N = (int)c->N;
    l0->R = S;
    l0->n = S * l0->N;
    l0->C = C;
    l0->off = c->noff.p;
    l0->cols = c->ncols.p;
    l0->vals = values_dev;
    l0->nnz = c->nnz_nodes;
    int rc = level_vectors(c, *l0);
    if (rc) return rc;
    if ((rc = near_nullspace(c, *l0, nullspace, B))) return rc;
    h->lv.push_back(std::move(l0));
    for (int l = 0;; ++l) {
        AmgLevel& L = *h->lv[l];
        if ((rc = level_diag(h.get(), l))) return rc;
        if (L.n <= AMG_MAX_COARSE_DOFS) break;
        if (h->lv.size() >= max_levels)
            return c->fail(FH_UNSUPPORTED, "fh_amg_create: the coarsest level has more than 4096 dofs (raise max_levels)");
        if ((rc = coarsen_symbolic(h.get(), l, theta))) return rc;
        if ((rc = level_vectors(c, *h->lv[l + 1]))) return rc;
        if ((rc = numeric_transfer(h.get(), l))) return rc;
    }
    if ((rc = factor_coarsest(h.get()))) return rc;
    *out = h.release();
    return FH_OK;
}

int fh_amg_update_values(fh_amg* h, const double* values_dev) {
    if (!h || !h->c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(h->device);
    if (!values_dev) return h->c->fail(FH_BAD_ARGUMENT, "fh_amg_update_values: null values");
    if (const int rc = amg_current(h, "fh_amg_update_values")) return rc;
    h->lv[0]->vals = values_dev;
    return numeric_all(h);
}

// touches the context only while it is alive (fh_destroy of the context clears h->c)
void fh_amg_destroy(fh_amg* h) {
    if (!h) return;
    DevGuard dev_guard_(h->device);
    if (h->c) {
        (void)hipStreamSynchronize(h->c->stream);
        if (h->c->amg == h) h->c->amg = nullptr;
    }
    delete h;
}

int fh_set_amg(fh_ctx* c, fh_amg* h) {
    if (!c) return FH_BAD_ARGUMENT;
    if (h && h->c != c) return c->fail(FH_BAD_ARGUMENT, "fh_set_amg: the hierarchy was made for another context");
    if (c->amg && c->amg != h) amg_orphan(c->amg);   // the one it replaces is orphaned: fh_amg_destroy will not touch this context
    c->amg = h;
    return FH_OK;
}

int fh_amg_set_smoother(fh_amg* h, uint32_t degree, double range, uint32_t eig_steps) {
    if (!h || !h->c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(h->device);
    if (degree < 1 || degree > 64 || !(range > 1.0) || eig_steps < 1 || eig_steps > 200)
        return h->c->fail(FH_BAD_ARGUMENT, "fh_amg_set_smoother: degree 1..64, range > 1, eig_steps 1..200");
    if (const int rc = amg_current(h, "fh_amg_set_smoother")) return rc;
    h->degree = degree;
    h->range = range;
    h->eig_steps = eig_steps;
    return numeric_all(h);
}

int fh_amg_apply_dev(fh_amg* h, const double* r_dev, double* z_dev) {
    if (!h || !h->c) return FH_BAD_ARGUMENT;
    fh_ctx* c = h->c;
    DevGuard dev_guard_(c->device);
    if (!r_dev || !z_dev || r_dev == z_dev) return c->fail(FH_BAD_ARGUMENT, "fh_amg_apply_dev: null or aliased vectors");
    int rc = amg_current(h, "fh_amg_apply_dev");
    if (rc) return rc;
    rc = vcycle(h, 0, r_dev, z_dev);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FH_OK;
}

int fh_amg_level_info(fh_amg* h, uint32_t level, uint64_t* num_dofs, uint64_t* nnz_blocks, uint32_t* block_size, double* lambda_max) {
    if (!h || !h->c) return FH_BAD_ARGUMENT;
    if (level >= h->lv.size()) return h->c->fail(FH_BAD_ARGUMENT, "fh_amg_level_info: no such level");
    const AmgLevel& L = *h->lv[level];
    if (num_dofs) *num_dofs = (uint64_t)L.n;
    if (nnz_blocks) *nnz_blocks = L.nnz;
    if (block_size) *block_size = (uint32_t)L.R;
    if (lambda_max) *lambda_max = L.lambda;
    return FH_OK;
}

int fh_amg_aggregates(fh_amg* h, uint32_t level, uint64_t* agg_of_node) {
    if (!h || !h->c) return FH_BAD_ARGUMENT;
    fh_ctx* c = h->c;
    DevGuard dev_guard_(c->device);
    if (level + 1 >= h->lv.size()) return c->fail(FH_BAD_ARGUMENT, "fh_amg_aggregates: the level has no coarser one");
    if (!agg_of_node) return c->fail(FH_BAD_ARGUMENT, "fh_amg_aggregates: null argument");
    const AmgLevel& L = *h->lv[level];
    std::vector<unsigned> a(L.N);
    if (L.N) HIP_TRY(c, hipMemcpyAsync(a.data(), L.agg.p, sizeof(unsigned) * L.N, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < L.N; ++i) agg_of_node[i] = a[i] == NONE ? UINT64_MAX : (uint64_t)a[i];
    return FH_OK;
}

int fh_amg_level_matrix(fh_amg* h, uint32_t level, int which, uint64_t* row_offsets, uint64_t* cols, double* vals, uint64_t* nnz) {
    if (!h || !h->c) return FH_BAD_ARGUMENT;
    fh_ctx* c = h->c;
    DevGuard dev_guard_(c->device);
    if (!nnz || which < 0 || which > 3) return c->fail(FH_BAD_ARGUMENT, "fh_amg_level_matrix: which is 0 (A), 1 (P), 2 (T) or 3 (B); nnz is required");
    const bool transfer = which == 1 || which == 2;
    if (level >= h->lv.size() || (transfer && level + 1 >= h->lv.size())) return c->fail(FH_BAD_ARGUMENT, "fh_amg_level_matrix: no such matrix");
    if (level == 0 && which == 0)
        if (const int rc = amg_current(h, "fh_amg_level_matrix")) return rc;
    const AmgLevel& L = *h->lv[level];
    const int R = L.R, N = L.N;
    if (which >= 2) {   // dense rows of C entries: T (block column agg(i), none on isolated nodes) or B
        std::vector<double> d((size_t)L.n * L.C);
        std::vector<unsigned> agg(which == 2 ? N : 0);
        if (L.n) HIP_TRY(c, hipMemcpyAsync(d.data(), which == 2 ? L.T.p : L.B.p, sizeof(double) * d.size(), hipMemcpyDeviceToHost, c->stream));
        if (which == 2 && N) HIP_TRY(c, hipMemcpyAsync(agg.data(), L.agg.p, sizeof(unsigned) * N, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        uint64_t total = 0;
        for (int i = 0; i < N; ++i) total += (which == 3 || agg[i] != NONE) ? (uint64_t)R * L.C : 0;
        *nnz = total;
        if (!row_offsets && !cols && !vals) return FH_OK;
        if (!row_offsets || !cols || !vals) return c->fail(FH_BAD_ARGUMENT, "fh_amg_level_matrix: give all three arrays or none");
        uint64_t p = 0;
        for (int i = 0; i < N; ++i)
            for (int a = 0; a < R; ++a) {
                row_offsets[(size_t)R * i + a] = p;
                if (which == 2 && agg[i] == NONE) continue;
                for (int k = 0; k < L.C; ++k) {
                    cols[p] = (which == 2 ? (uint64_t)agg[i] * L.C : 0) + k;
                    vals[p++] = d[((size_t)R * i + a) * L.C + k];
                }
            }
        row_offsets[(size_t)R * N] = p;
        return FH_OK;
    }
    const int Cb = which ? L.C : L.R;
    const unsigned* d_off = which ? L.p_off.p : L.off;
    const unsigned* d_cols = which ? L.p_cols.p : L.cols;
    const double* d_vals = which ? L.p_vals.p : L.vals;
    std::vector<unsigned> off(N + 1, 0);
    if (N) HIP_TRY(c, hipMemcpyAsync(off.data(), d_off, sizeof(unsigned) * (N + 1), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const uint64_t total = (uint64_t)off[N] * R * Cb;
    *nnz = total;
    if (!row_offsets && !cols && !vals) return FH_OK;
    if (!row_offsets || !cols || !vals) return c->fail(FH_BAD_ARGUMENT, "fh_amg_level_matrix: give all three arrays or none");
    std::vector<unsigned> bc(off[N]);
    if (off[N]) {
        HIP_TRY(c, hipMemcpyAsync(bc.data(), d_cols, sizeof(unsigned) * bc.size(), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(vals, d_vals, sizeof(double) * total, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    uint64_t p = 0;
    for (int i = 0; i < N; ++i) {
        const unsigned cnt = off[i + 1] - off[i];
        for (int a = 0; a < R; ++a) {
            row_offsets[(size_t)R * i + a] = p;
            for (unsigned kk = 0; kk < cnt; ++kk)
                for (int b = 0; b < Cb; ++b) cols[p++] = (uint64_t)Cb * bc[off[i] + kk] + b;
        }
    }
    row_offsets[(size_t)R * N] = p;
    return FH_OK;
}

}  // extern "C"
