#pragma once
// Kernels of the smoothed-aggregation hierarchy (engine_amg.hip).  Matrices are node-block CSR: block row i holds cnt = off[i + 1] - off[i]
// blocks of R x C, and entry (a, b) of its kk-th block sits at vals[R C off[i] + a C cnt + C kk + b] -- the layout of the assembled values,
// i.e. the scalar CSR of the R rows of the node.  Every floating-point sum has a fixed order and no kernel uses floating-point atomics;
// integer atomics only count and place, and every placement is sorted afterwards, so setup and V-cycle repeat bit for bit.
#include <hip/hip_runtime.h>

namespace fenris_hip_amg {

constexpr unsigned NONE = 0xffffffffu;
constexpr int MAX_B = 6;          // largest block edge: nb <= 6
constexpr int SPGEMM_CAP = 512;   // longest row of a Galerkin product (more: the setup reports FH_UNSUPPORTED)

// the priority of node i in the aggregation: a fixed 31-bit hash of i above the index (ties broken by the index)
__device__ __forceinline__ unsigned long long amg_key(unsigned i) {
    unsigned h = i;
    h ^= h >> 16;
    h *= 0x7feb352du;
    h ^= h >> 15;
    h *= 0x846ca68bu;
    h ^= h >> 16;
    return ((unsigned long long)(h & 0x7fffffffu) << 32) | i;
}

// point diagonal (a zero diagonal becomes +inf, so that D^-1 = 0 there) and ||A_ii||_F per node
static __global__ void __launch_bounds__(256) k_amg_diag(int N, int R, const unsigned* off, const unsigned* cols, const double* vals, double* dnorm,
                                                         double* diag) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
        const unsigned r0 = off[i], cnt = off[i + 1] - r0;
        unsigned kk = 0;
        while (kk < cnt && cols[r0 + kk] != (unsigned)i) ++kk;
        double s = 0.0;
        for (int a = 0; a < R; ++a) {
            double d = 0.0;
            if (kk < cnt) {
                const double* row = vals + (size_t)R * R * r0 + (size_t)a * R * cnt + (size_t)R * kk;
                for (int b = 0; b < R; ++b) s = fma(row[b], row[b], s);
                d = row[a];
            }
            diag[(size_t)R * i + a] = d == 0.0 ? __builtin_inf() : d;
        }
        dnorm[i] = sqrt(s);
    }
}

// strong[k] for every block of the pattern; iso[i]: no nonzero off-diagonal block in row i
static __global__ void __launch_bounds__(256) k_amg_strength(int N, int R, const unsigned* off, const unsigned* cols, const double* vals,
                                                             const double* dnorm, double theta, unsigned char* strong, unsigned char* iso) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
        const unsigned r0 = off[i], cnt = off[i + 1] - r0;
        bool any = false;
        for (unsigned kk = 0; kk < cnt; ++kk) {
            const unsigned j = cols[r0 + kk];
            double s = 0.0;
            if (j != (unsigned)i)
                for (int a = 0; a < R; ++a) {
                    const double* row = vals + (size_t)R * R * r0 + (size_t)a * R * cnt + (size_t)R * kk;
                    for (int b = 0; b < R; ++b) s = fma(row[b], row[b], s);
                }
            const double nf = sqrt(s);
            any = any || nf > 0.0;
            strong[r0 + kk] = (j != (unsigned)i && nf > 0.0 && nf >= theta * sqrt(dnorm[i] * dnorm[j])) ? 1 : 0;
        }
        iso[i] = any ? 0 : 0xff;   // (all ones: mg_estimate_lambda reads the flags as Dirichlet bytes, every component of the block held)
    }
}

// the starting state of the independent set: isolated (3) or undecided (0); *any = 1 when some node is isolated
static __global__ void __launch_bounds__(256) k_amg_state_init(int N, const unsigned char* iso, unsigned char* state, int* any) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
        state[i] = iso[i] ? 3 : 0;
        if (iso[i]) *any = 1;
    }
}

// ---- distance-2 maximal independent set.  state: 0 undecided, 1 root, 2 out, 3 isolated.  value: key + 1 (undecided), ~0 (root), 0 else
static __global__ void __launch_bounds__(256) k_amg_mis_value(int N, const unsigned char* state, unsigned long long* v) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
        const unsigned char s = state[i];
        v[i] = s == 0 ? amg_key((unsigned)i) + 1 : (s == 1 ? ~0ull : 0ull);
    }
}

// vout[i] = max of vin over i and its strong neighbours
static __global__ void __launch_bounds__(256) k_amg_mis_max(int N, const unsigned* off, const unsigned* cols, const unsigned char* strong,
                                                            const unsigned long long* vin, unsigned long long* vout) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
        unsigned long long m = vin[i];
        for (unsigned k = off[i]; k < off[i + 1]; ++k)
            if (strong[k]) m = max(m, vin[cols[k]]);
        vout[i] = m;
    }
}

// an undecided node that holds the largest value within distance 2 becomes a root; one with a root within distance 2 is out
static __global__ void __launch_bounds__(256) k_amg_mis_update(int N, unsigned char* state, const unsigned long long* v2, int* undecided) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
        if (state[i] != 0) continue;
        const unsigned long long m = v2[i];
        if (m == amg_key((unsigned)i) + 1) state[i] = 1;
        else if (m == ~0ull) state[i] = 2;
        else *undecided = 1;
    }
}

static __global__ void __launch_bounds__(256) k_amg_root_flags(int N, const unsigned char* state, unsigned* flags) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i <= N; i += gridDim.x * blockDim.x) flags[i] = (i < N && state[i] == 1) ? 1u : 0u;
}

// roots take their rank among the roots; every other non-isolated node joins the adjacent root of highest priority (NONE if there is none)
static __global__ void __launch_bounds__(256) k_amg_join(int N, const unsigned* off, const unsigned* cols, const unsigned char* strong,
                                                         const unsigned char* state, const unsigned* root_rank, unsigned* agg) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
        const unsigned char s = state[i];
        unsigned a = NONE;
        if (s == 1) {
            a = root_rank[i];
        } else if (s != 3) {
            unsigned long long best = 0;
            for (unsigned k = off[i]; k < off[i + 1]; ++k) {
                const unsigned j = cols[k];
                if (!strong[k] || state[j] != 1) continue;
                const unsigned long long kj = amg_key(j) + 1;
                if (kj > best) { best = kj; a = root_rank[j]; }
            }
        }
        agg[i] = a;
    }
}

// one sweep: a non-isolated node still without an aggregate joins the one of its aggregated strong neighbour of highest priority
static __global__ void __launch_bounds__(256) k_amg_sweep(int N, const unsigned* off, const unsigned* cols, const unsigned char* strong,
                                                          const unsigned char* state, const unsigned* agg_in, unsigned* agg_out, int* left) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
        unsigned a = agg_in[i];
        if (a == NONE && state[i] != 3) {
            unsigned long long best = 0;
            for (unsigned k = off[i]; k < off[i + 1]; ++k) {
                const unsigned j = cols[k];
                if (!strong[k] || agg_in[j] == NONE) continue;
                const unsigned long long kj = amg_key(j) + 1;
                if (kj > best) { best = kj; a = agg_in[j]; }
            }
            if (a == NONE) *left = 1;
        }
        agg_out[i] = a;
    }
}

// ---- stable counting sort of items 0..m-1 by key (NONE: dropped): counts, (scan), placement, then each segment sorted by item index
static __global__ void __launch_bounds__(256) k_amg_count_keys(long long m, const unsigned* key, unsigned* cnt) {
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < m; t += (long long)gridDim.x * blockDim.x)
        if (key[t] != NONE) atomicAdd(&cnt[key[t]], 1u);
}
static __global__ void __launch_bounds__(256) k_amg_place(long long m, const unsigned* key, const unsigned* seg_off, unsigned* cursor, unsigned* item) {
    for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < m; t += (long long)gridDim.x * blockDim.x)
        if (key[t] != NONE) item[seg_off[key[t]] + atomicAdd(&cursor[key[t]], 1u)] = (unsigned)t;
}
static __global__ void __launch_bounds__(256) k_amg_sort_segments(int K, const unsigned* seg_off, unsigned* item) {
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < K; s += gridDim.x * blockDim.x) {
        const unsigned lo = seg_off[s], hi = seg_off[s + 1];
        for (unsigned p = lo + 1; p < hi; ++p) {
            const unsigned v = item[p];
            unsigned q = p;
            while (q > lo && item[q - 1] > v) { item[q] = item[q - 1]; --q; }
            item[q] = v;
        }
    }
}

// dst[q] = src[idx[q]]
static __global__ void __launch_bounds__(256) k_amg_gather(long long m, const unsigned* idx, const unsigned* src, unsigned* dst) {
    for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < m; q += (long long)gridDim.x * blockDim.x) dst[q] = src[idx[q]];
}

// row[k] = the row of entry k
static __global__ void __launch_bounds__(256) k_amg_fill_rows(int N, const unsigned* off, unsigned* row) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x)
        for (unsigned k = off[i]; k < off[i + 1]; ++k) row[k] = (unsigned)i;
}

// ---- near-nullspace of the fine level
static __global__ void __launch_bounds__(256) k_amg_coord_partials(int N, int d, const double* verts, double* partial /* gridDim.x x 3 */) {
    __shared__ double red[3][256];
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x)
        for (int k = 0; k < d; ++k) s[k] += verts[(size_t)d * i + k];
    for (int k = 0; k < 3; ++k) red[k][threadIdx.x] = s[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
            for (int k = 0; k < 3; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        for (int k = 0; k < 3; ++k) partial[3 * blockIdx.x + k] = red[k][0];
}

// rigid-body modes about the centroid c: translations, then (2D) the rotation (-y, x), (3D) the rotations about x, y, z
static __global__ void __launch_bounds__(256) k_amg_rigid_body(int N, int d, const double* verts, double cx, double cy, double cz, double* B) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
        const double x = verts[(size_t)d * i] - cx, y = verts[(size_t)d * i + 1] - cy;
        if (d == 2) {
            double* b = B + (size_t)6 * i;   // 2 rows x 3 columns
            b[0] = 1.0; b[1] = 0.0; b[2] = -y;
            b[3] = 0.0; b[4] = 1.0; b[5] = x;
        } else {
            const double z = verts[(size_t)d * i + 2] - cz;
            double* b = B + (size_t)18 * i;  // 3 rows x 6 columns
            const double m[18] = {1.0, 0.0, 0.0, 0.0, z, -y,
                                  0.0, 1.0, 0.0, -z, 0.0, x,
                                  0.0, 0.0, 1.0, y, -x, 0.0};
            for (int k = 0; k < 18; ++k) b[k] = m[k];
        }
    }
}

static __global__ void __launch_bounds__(256) k_amg_constant(int N, int s, double* B) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x)
        for (int a = 0; a < s; ++a)
            for (int k = 0; k < s; ++k) B[((size_t)s * i + a) * s + k] = a == k ? 1.0 : 0.0;
}

// ---- tentative prolongator: per aggregate J (members in ascending node order), modified Gram-Schmidt of its rows of B (R rows per node,
// C columns); T (zeroed before) gets Q, Bc gets R (C x C, row-major at block J)
static __global__ void __launch_bounds__(64) k_amg_tentative(int nagg, int R, int C, const unsigned* agg_off, const unsigned* members, const double* B,
                                                             double* T, double* Bc) {
    for (int J = blockIdx.x * blockDim.x + threadIdx.x; J < nagg; J += gridDim.x * blockDim.x) {
        const unsigned lo = agg_off[J], hi = agg_off[J + 1];
        double Rm[MAX_B][MAX_B];
        for (int j = 0; j < C; ++j)
            for (int k = 0; k < C; ++k) Rm[j][k] = 0.0;
        for (unsigned m = lo; m < hi; ++m)
            for (int a = 0; a < R; ++a) {
                const size_t row = (size_t)R * members[m] + a;
                for (int k = 0; k < C; ++k) T[row * C + k] = B[row * C + k];
            }
        for (int k = 0; k < C; ++k) {
            double n0 = 0.0;
            for (unsigned m = lo; m < hi; ++m)
                for (int a = 0; a < R; ++a) {
                    const double v = T[((size_t)R * members[m] + a) * C + k];
                    n0 = fma(v, v, n0);
                }
            for (int j = 0; j < k; ++j) {
                double r = 0.0;
                for (unsigned m = lo; m < hi; ++m)
                    for (int a = 0; a < R; ++a) {
                        const size_t row = ((size_t)R * members[m] + a) * C;
                        r = fma(T[row + j], T[row + k], r);
                    }
                for (unsigned m = lo; m < hi; ++m)
                    for (int a = 0; a < R; ++a) {
                        const size_t row = ((size_t)R * members[m] + a) * C;
                        T[row + k] = fma(-r, T[row + j], T[row + k]);
                    }
                Rm[j][k] = r;
            }
            double n1 = 0.0;
            for (unsigned m = lo; m < hi; ++m)
                for (int a = 0; a < R; ++a) {
                    const double v = T[((size_t)R * members[m] + a) * C + k];
                    n1 = fma(v, v, n1);
                }
            n0 = sqrt(n0);
            n1 = sqrt(n1);
            const bool drop = !(n1 > 1e-10 * n0);
            for (unsigned m = lo; m < hi; ++m)
                for (int a = 0; a < R; ++a) {
                    double& v = T[((size_t)R * members[m] + a) * C + k];
                    v = drop ? 0.0 : v / n1;
                }
            Rm[k][k] = drop ? 0.0 : n1;
        }
        for (int j = 0; j < C; ++j)
            for (int k = 0; k < C; ++k) Bc[((size_t)C * J + j) * C + k] = Rm[j][k];
    }
}

// ---- the pattern of P: block row i holds the distinct aggregates of the nodes of A's row i (none for an unaggregated node), ascending.
// out null: cnt[i] only; else the columns at p_off[i]
static __global__ void __launch_bounds__(256) k_amg_p_pattern(int N, const unsigned* off, const unsigned* cols, const unsigned* agg, unsigned* cnt,
                                                              const unsigned* p_off, unsigned* out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
        unsigned c = 0;
        if (agg[i] != NONE) {
            const unsigned lo = off[i], hi = off[i + 1];
            for (unsigned k = lo; k < hi; ++k) {
                const unsigned g = agg[cols[k]];
                if (g == NONE) continue;
                bool seen = false;
                for (unsigned q = lo; q < k && !seen; ++q) seen = agg[cols[q]] == g;
                if (seen) continue;
                if (out) {   // insertion into the sorted prefix
                    unsigned p = p_off[i] + c;
                    while (p > p_off[i] && out[p - 1] > g) { out[p] = out[p - 1]; --p; }
                    out[p] = g;
                }
                ++c;
            }
        }
        if (!out) cnt[i] = c;
    }
}

// P = (I - omega D^-1 A) T, one thread per block of P: the sum over A's row in pattern order, b ascending
static __global__ void __launch_bounds__(256) k_amg_p_values(long long nnzP, int R, int C, const unsigned* p_row, const unsigned* p_off,
                                                             const unsigned* p_cols, const unsigned* off, const unsigned* cols, const double* vals,
                                                             const unsigned* agg, const double* T, const double* diag, double omega, double* pv) {
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < nnzP; e += (long long)gridDim.x * blockDim.x) {
        const unsigned i = p_row[e], J = p_cols[e];
        const unsigned r0 = off[i], cnt = off[i + 1] - r0;
        const unsigned kp = (unsigned)e - p_off[i], cntP = p_off[i + 1] - p_off[i];
        double acc[MAX_B][MAX_B];
        for (int a = 0; a < R; ++a)
            for (int c = 0; c < C; ++c) acc[a][c] = 0.0;
        for (unsigned kk = 0; kk < cnt; ++kk) {
            const unsigned j = cols[r0 + kk];
            if (agg[j] != J) continue;
            for (int a = 0; a < R; ++a) {
                const double* arow = vals + (size_t)R * R * r0 + (size_t)a * R * cnt + (size_t)R * kk;
                for (int b = 0; b < R; ++b) {
                    const double* t = T + ((size_t)R * j + b) * C;
                    for (int c = 0; c < C; ++c) acc[a][c] = fma(arow[b], t[c], acc[a][c]);
                }
            }
        }
        const bool own = agg[i] == J;
        for (int a = 0; a < R; ++a) {
            const double dinv = 1.0 / diag[(size_t)R * i + a];
            for (int c = 0; c < C; ++c) {
                const double t = own ? T[((size_t)R * i + a) * C + c] : 0.0;
                pv[(size_t)R * C * p_off[i] + (size_t)a * C * cntP + (size_t)C * kp + c] = t - omega * (dinv * acc[a][c]);
            }
        }
    }
}

// P^T's blocks (C x R) from P's (R x C): entry q of P^T is entry src[q] of P
static __global__ void __launch_bounds__(256) k_amg_transpose_values(long long nnz, int R, int C, const unsigned* t_row, const unsigned* t_off,
                                                                     const unsigned* src, const unsigned* p_row, const unsigned* p_off,
                                                                     const double* pv, double* tv) {
    for (long long q = blockIdx.x * (long long)blockDim.x + threadIdx.x; q < nnz; q += (long long)gridDim.x * blockDim.x) {
        const unsigned J = t_row[q], e = src[q], i = p_row[e];
        const unsigned kq = (unsigned)q - t_off[J], cntT = t_off[J + 1] - t_off[J];
        const unsigned kp = e - p_off[i], cntP = p_off[i + 1] - p_off[i];
        for (int c = 0; c < C; ++c)
            for (int a = 0; a < R; ++a)
                tv[(size_t)C * R * t_off[J] + (size_t)c * R * cntT + (size_t)R * kq + a] = pv[(size_t)R * C * p_off[i] + (size_t)a * C * cntP + (size_t)C * kp + c];
    }
}

// ---- sparse product pattern: row i of X Y holds the distinct columns of Y's rows at X's row i, ascending (a sorted list of at most
// SPGEMM_CAP).  out null: cnt[i]; else the columns at z_off[i].  *overflow = 1 on a longer row.
static __global__ void __launch_bounds__(256) k_amg_spgemm_pattern(int N, const unsigned* x_off, const unsigned* x_cols, const unsigned* y_off,
                                                                   const unsigned* y_cols, unsigned* cnt, const unsigned* z_off, unsigned* out,
                                                                   int* overflow) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
        unsigned list[SPGEMM_CAP];
        int n = 0;
        bool over = false;
        for (unsigned k = x_off[i]; k < x_off[i + 1] && !over; ++k) {
            const unsigned j = x_cols[k];
            for (unsigned q = y_off[j]; q < y_off[j + 1]; ++q) {
                const unsigned g = y_cols[q];
                int lo = 0, hi = n;   // first position >= g
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (list[mid] < g) lo = mid + 1; else hi = mid;
                }
                if (lo < n && list[lo] == g) continue;
                if (n == SPGEMM_CAP) { over = true; break; }
                for (int p = n; p > lo; --p) list[p] = list[p - 1];
                list[lo] = g;
                ++n;
            }
        }
        if (over) { *overflow = 1; n = 0; }
        if (out) {
            for (int p = 0; p < n; ++p) out[z_off[i] + p] = list[p];
        } else {
            cnt[i] = (unsigned)n;
        }
    }
}

// Z = X Y block by block: X blocks RA x K, Y blocks K x CB, Z blocks RA x CB; the sum over X's row in pattern order, inner index ascending.
// upper_only: blocks left of the diagonal are skipped (k_amg_mirror fills them)
static __global__ void __launch_bounds__(256) k_amg_spgemm_values(long long nnzZ, int RA, int K, int CB, const unsigned* z_row, const unsigned* z_off,
                                                                  const unsigned* z_cols, const unsigned* x_off, const unsigned* x_cols,
                                                                  const double* xv, const unsigned* y_off, const unsigned* y_cols, const double* yv,
                                                                  double* zv, int upper_only) {
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < nnzZ; e += (long long)gridDim.x * blockDim.x) {
        const unsigned i = z_row[e], J = z_cols[e];
        if (upper_only && J < i) continue;
        const unsigned kz = (unsigned)e - z_off[i], cntZ = z_off[i + 1] - z_off[i];
        const unsigned x0 = x_off[i], cntX = x_off[i + 1] - x0;
        double acc[MAX_B][MAX_B];
        for (int a = 0; a < RA; ++a)
            for (int c = 0; c < CB; ++c) acc[a][c] = 0.0;
        for (unsigned kk = 0; kk < cntX; ++kk) {
            const unsigned j = x_cols[x0 + kk];
            const unsigned y0 = y_off[j], y1 = y_off[j + 1];
            unsigned lo = y0, hi = y1;
            while (lo < hi) {
                const unsigned mid = (lo + hi) >> 1;
                if (y_cols[mid] < J) lo = mid + 1; else hi = mid;
            }
            if (lo == y1 || y_cols[lo] != J) continue;
            const unsigned ky = lo - y0, cntY = y1 - y0;
            for (int a = 0; a < RA; ++a) {
                const double* xr = xv + (size_t)RA * K * x0 + (size_t)a * K * cntX + (size_t)K * kk;
                for (int b = 0; b < K; ++b) {
                    const double* yr = yv + (size_t)K * CB * y0 + (size_t)b * CB * cntY + (size_t)CB * ky;
                    for (int c = 0; c < CB; ++c) acc[a][c] = fma(xr[b], yr[c], acc[a][c]);
                }
            }
        }
        for (int a = 0; a < RA; ++a)
            for (int c = 0; c < CB; ++c) zv[(size_t)RA * CB * z_off[i] + (size_t)a * CB * cntZ + (size_t)CB * kz + c] = acc[a][c];
    }
}

// exact symmetry of a square-block matrix whose upper blocks are formed: block (i, J), J < i, is the transpose of block (J, i), and the
// lower triangle of a diagonal block is its upper one mirrored
static __global__ void __launch_bounds__(256) k_amg_mirror(long long nnz, int B, const unsigned* row, const unsigned* off, const unsigned* cols,
                                                           double* v) {
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < nnz; e += (long long)gridDim.x * blockDim.x) {
        const unsigned i = row[e], J = cols[e];
        const unsigned ki = (unsigned)e - off[i], cntI = off[i + 1] - off[i];
        double* dst = v + (size_t)B * B * off[i] + (size_t)B * ki;
        if (J == i) {
            for (int a = 1; a < B; ++a)
                for (int b = 0; b < a; ++b) dst[(size_t)a * B * cntI + b] = dst[(size_t)b * B * cntI + a];
        } else if (J < i) {
            unsigned lo = off[J], hi = off[J + 1];
            while (lo < hi) {
                const unsigned mid = (lo + hi) >> 1;
                if (cols[mid] < i) lo = mid + 1; else hi = mid;
            }
            if (lo == off[J + 1] || cols[lo] != i) continue;   // (the pattern of P^T A P is symmetric)
            const unsigned kj = lo - off[J], cntJ = off[J + 1] - off[J];
            const double* src = v + (size_t)B * B * off[J] + (size_t)B * kj;
            for (int a = 0; a < B; ++a)
                for (int b = 0; b < B; ++b) dst[(size_t)a * B * cntI + b] = src[(size_t)b * B * cntJ + a];
        }
    }
}

// ---- V-cycle: y (+)= M x with M of R x C blocks, one thread per scalar row, the row's blocks in pattern order and b ascending
template <int C>
static __global__ void __launch_bounds__(256) k_amg_spmv(int rows, int R, const unsigned* off, const unsigned* cols, const double* vals, const double* x,
                                                         double* y, int accumulate) {
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < rows; t += gridDim.x * blockDim.x) {
        const int i = t / R, a = t - i * R;
        const unsigned r0 = off[i], cnt = off[i + 1] - r0;
        const double* v = vals + (size_t)R * C * r0 + (size_t)a * C * cnt;
        double acc = 0.0;
        for (unsigned kk = 0; kk < cnt; ++kk) {
            const double* xj = x + (size_t)C * cols[r0 + kk];
#pragma unroll
            for (int b = 0; b < C; ++b) acc = fma(v[C * kk + b], xj[b], acc);
        }
        y[t] = accumulate ? y[t] + acc : acc;
    }
}

// the inverse of the diagonal block of every isolated node (R x R, row-major at inv + R R i) by Cholesky, W = L^-1, W^T W (exactly
// symmetric); a pivot at most 1e-14 of its diagonal (or a zero diagonal) leaves that dof out, with zero rows and columns
static __global__ void __launch_bounds__(64) k_amg_iso_inverse(int N, int R, const unsigned* off, const unsigned* cols, const double* vals,
                                                               const unsigned char* iso, double* inv) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < N; i += gridDim.x * blockDim.x) {
        if (!iso[i]) continue;
        const unsigned r0 = off[i], cnt = off[i + 1] - r0;
        unsigned kk = 0;
        while (kk < cnt && cols[r0 + kk] != (unsigned)i) ++kk;
        double L[MAX_B][MAX_B], W[MAX_B][MAX_B];
        bool out[MAX_B];
        for (int a = 0; a < R; ++a)
            for (int b = 0; b < R; ++b) {
                L[a][b] = kk < cnt ? vals[(size_t)R * R * r0 + (size_t)a * R * cnt + (size_t)R * kk + b] : 0.0;
                W[a][b] = 0.0;
            }
        for (int j = 0; j < R; ++j) {
            const double d0 = L[j][j];
            double sj = d0;
            for (int k = 0; k < j; ++k) sj -= L[j][k] * L[j][k];
            out[j] = !(sj > 1e-14 * d0);
            if (out[j]) {
                for (int a = j; a < R; ++a) L[a][j] = 0.0;
                continue;
            }
            const double djj = sqrt(sj);
            L[j][j] = djj;
            for (int a = j + 1; a < R; ++a) {
                double t = L[a][j];
                for (int k = 0; k < j; ++k) t -= L[a][k] * L[j][k];
                L[a][j] = t / djj;
            }
        }
        for (int c = 0; c < R; ++c) {
            if (out[c]) continue;
            W[c][c] = 1.0 / L[c][c];
            for (int a = c + 1; a < R; ++a) {
                if (out[a]) continue;
                double t = 0.0;
                for (int k = c; k < a; ++k) t += L[a][k] * W[k][c];
                W[a][c] = -t / L[a][a];
            }
        }
        double* o = inv + (size_t)R * R * i;
        for (int a = 0; a < R; ++a)
            for (int b = a; b < R; ++b) {
                double t = 0.0;
                for (int k = b; k < R; ++k) t += W[k][a] * W[k][b];
                o[a * R + b] = t;
                o[b * R + a] = t;
            }
    }
}

// x_i = A_ii^-1 b_i on the isolated nodes
static __global__ void __launch_bounds__(256) k_amg_iso_apply(int N, int R, const unsigned char* iso, const double* inv, const double* b, double* x) {
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < N * R; t += gridDim.x * blockDim.x) {
        const int i = t / R, a = t - i * R;
        if (!iso[i]) continue;
        const double* o = inv + (size_t)R * R * i + (size_t)a * R;
        double acc = 0.0;
        for (int c = 0; c < R; ++c) acc = fma(o[c], b[(size_t)R * i + c], acc);
        x[t] = acc;
    }
}

// r = b - t
static __global__ void __launch_bounds__(256) k_amg_residual(int n, const double* b, const double* t, double* r) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) r[i] = b[i] - t[i];
}

// per-workgroup partials of x . y (the eigenvalue estimate)
static __global__ void __launch_bounds__(256) k_amg_dot_partials(int n, const double* x, const double* y, double* partial) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) s = fma(x[i], y[i], s);
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

}  // namespace fenris_hip_amg
