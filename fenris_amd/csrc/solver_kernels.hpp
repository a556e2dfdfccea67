// Callers of the assembly path that keep K on the device: Jacobi-preconditioned conjugate
// gradients on the node-blocked CSR (fenris-sparse/src/cg.rs:196-474 as driven by solve_linear_system,
// tests/convergence_tests/poisson_mms_common.rs:142-163) and the L2 / H1 error integrals (src/error.rs:287-372).
// All reductions are two-stage: per-workgroup partial sums in a fixed order, summed in workgroup order by the
// host => bitwise reproducible runs (no floating-point atomics).
#pragma once
#include <hip/hip_runtime.h>

#include "assemble_kernels.hpp"
#include "device_common.hpp"
#include "element_pass.hpp"
#include "material.hpp"

namespace fenris_hip {

// sum over the 64 lanes of a wavefront (butterfly, every lane gets the total)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Sum of K per-thread values over a 256-thread workgroup, in a fixed order; thread 0 stores to out[0..K).
template <int K>
__device__ __forceinline__ void block_sum_store(double (&v)[K], double* out) {
    __shared__ double part[4][K];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double s = wave_sum(v[k]);
        if (lane == 0) part[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) out[k] = (part[0][k] + part[1][k]) + (part[2][k] + part[3][k]);
}

// `count` groups of K partials -> gridDim.x groups of K sums, each over one contiguous part of them, in a fixed order: the SpMV and the vector kernels of
// the CG loop launch short-lived workgroups (see spmv_launch) and leave K partials per workgroup; the host sums what this kernel leaves
template <int K>
static __global__ void __launch_bounds__(256) k_sum_partial_ranges(const double* in, long long count, double* out) {
    const long long per = (count + gridDim.x - 1) / gridDim.x;
    const long long lo = per * blockIdx.x, hi = min(count, lo + per);
    double s[K];
#pragma unroll
    for (int j = 0; j < K; ++j) s[j] = 0.0;
    for (long long k = lo + threadIdx.x; k < hi; k += 256)
#pragma unroll
        for (int j = 0; j < K; ++j) s[j] += in[K * k + j];
    block_sum_store<K>(s, out + K * blockIdx.x);
}

// y = A x on the node-blocked CSR: the S rows of node i are contiguous, each S * cnt long, and share the
// node-level column list (global.rs:100-118).  One wavefront per node (grid-stride); lanes stride over the
// row entries, S row sums per lane, butterfly reduction.  Optionally the partial of  x . y  per workgroup.
template <int S>
__global__ void __launch_bounds__(256) k_spmv_blocked(int num_nodes, const unsigned* noff, const unsigned* ncols, const double* vals,
                                                      const double* x, double* y, double* dot_partial) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double dot[1] = {0.0};
    for (int i = blockIdx.x * 4 + wave; i < num_nodes; i += gridDim.x * 4) {
        const unsigned r0 = noff[i], cnt = noff[i + 1] - r0;
        const int len = S * (int)cnt;
        const double* row = vals + (size_t)S * S * r0;
        double acc[S];
#pragma unroll
        for (int a = 0; a < S; ++a) acc[a] = 0.0;
        for (int t = lane; t < len; t += 64) {
            const double xv = x[(size_t)S * ncols[r0 + t / S] + t % S];
#pragma unroll
            for (int a = 0; a < S; ++a) acc[a] = fma(row[(size_t)a * len + t], xv, acc[a]);
        }
#pragma unroll
        for (int a = 0; a < S; ++a) {
            const double s = wave_sum(acc[a]);
            if (lane == 0) {
                y[(size_t)S * i + a] = s;
                dot[0] = fma(x[(size_t)S * i + a], s, dot[0]);
            }
        }
    }
    if (dot_partial) block_sum_store<1>(dot, dot_partial + blockIdx.x);
}

// sum over the 32 lanes of a half wavefront by DPP moves on the vector pipe (xor 1, 2, 4, 8 inside each row of 16 lanes, then row_bcast:15 hands the
// total of rows 0 / 2 to rows 1 / 3): the lanes 16 .. 31 of the half hold the total.  Through __shfl_xor the same sum is ten ds_bpermute per value --
// LDS-pipe instructions; the SpMV issued sixty of them per four nodes.
__device__ __forceinline__ double half_sum_hi(double v) {
    v += dpp_quad_full<0xB1>(v);
    v += dpp_quad_full<0x4E>(v);
    v += dpp_xor4(v);
    {   // row_ror:8 = lane ^ 8 inside a row of 16
        const long long b = __builtin_bit_cast(long long, v);
        const int lo = __builtin_amdgcn_mov_dpp((int)b, 0x128, 0xF, 0xF, true), hi = __builtin_amdgcn_mov_dpp((int)(b >> 32), 0x128, 0xF, 0xF, true);
        v += __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned long long)(unsigned)lo);
    }
    {   // row_bcast:15 into rows 1 and 3 (row mask 0xA); rows 0 and 2 add zero
        const long long b = __builtin_bit_cast(long long, v);
        const int lo = __builtin_amdgcn_update_dpp(0, (int)b, 0x142, 0xA, 0xF, false), hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), 0x142, 0xA, 0xF, false);
        v += __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned long long)(unsigned)lo);
    }
    return v;
}

// The same product for patterns whose node rows hold at most 32 column blocks (Quad4 9, Tet4 ~15, Hex8 27): HALF a wavefront per
// node, one lane per column block -- the lane fetches its column index, the S entries of x and its S x S block (S runs of S
// contiguous doubles; neighbouring lanes read neighbouring runs) -- and two node pairs per wavefront in flight.  The
// one-wavefront-per-node form above walks a row of 81 entries in two trips of 64 lanes behind three dependent fetches (row offset
// -> column index -> x): with 32 wavefronts per CU that chain, not the memory system, set its rate (3.2 TB/s on Hex8 216^3).
template <int S, int UN = 2>
__global__ void __launch_bounds__(256) k_spmv_blocked_half(int num_nodes, const unsigned* noff, const unsigned* ncols, const double* vals,
                                                           const double* x, double* y, double* dot_partial) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, hl = lane & 31;
    // UN: node pairs in flight per wavefront
    double dot[1] = {0.0};
    const int stride = gridDim.x * 4 * 2 * UN;
    for (int base = (blockIdx.x * 4 + wave) * 2 * UN; base < num_nodes; base += stride) {
        double acc[UN][S];
        int node[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            node[u] = base + 2 * u + half;
            const int nc = min(node[u], num_nodes - 1);
            const unsigned r0 = noff[nc], cnt = noff[nc + 1] - r0;
            const bool act = node[u] < num_nodes && (unsigned)hl < cnt;
#pragma unroll
            for (int a = 0; a < S; ++a) acc[u][a] = 0.0;
            if (act) {
                const unsigned col = ncols[r0 + hl];
                double xv[S];
#pragma unroll
                for (int c = 0; c < S; ++c) xv[c] = x[(size_t)S * col + c];
                const double* blk = vals + (size_t)S * S * r0 + (size_t)S * hl;
                if constexpr (S == 3) {
                    // a row of the block is 24 bytes at an 8-byte boundary: one 16-byte and one 8-byte load (six load instructions per lane instead of nine)
                    typedef double f64x2_u8s __attribute__((ext_vector_type(2), aligned(8)));
#pragma unroll
                    for (int a = 0; a < S; ++a) {
                        const double* rw = blk + (size_t)a * S * cnt;
                        const f64x2_u8s v01 = *reinterpret_cast<const f64x2_u8s*>(rw);
                        const double v2 = rw[2];
                        acc[u][a] = fma(v01.x, xv[0], acc[u][a]);
                        acc[u][a] = fma(v01.y, xv[1], acc[u][a]);
                        acc[u][a] = fma(v2, xv[2], acc[u][a]);
                    }
                } else {
#pragma unroll
                for (int a = 0; a < S; ++a)
#pragma unroll
                    for (int c = 0; c < S; ++c) acc[u][a] = fma(blk[(size_t)a * S * cnt + c], xv[c], acc[u][a]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < UN; ++u)
#pragma unroll
            for (int a = 0; a < S; ++a) {
                const double s = half_sum_hi(acc[u][a]);   // over the half wavefront: its lanes 16 .. 31 hold the sum
                if (hl == 16 && node[u] < num_nodes) {
                    y[(size_t)S * node[u] + a] = s;
                    dot[0] = fma(x[(size_t)S * node[u] + a], s, dot[0]);
                }
            }
    }
    if (dot_partial) block_sum_store<1>(dot, dot_partial + blockIdx.x);
}

// 1 / diagonal of the blocked CSR (matrix.diagonal_as_csr() + recip, poisson_mms_common.rs:148-151)
template <int S>
__global__ void __launch_bounds__(256) k_inverse_diagonal(int num_nodes, const unsigned* noff, const unsigned* ncols, const double* vals,
                                                          double* dinv) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= S * num_nodes) return;
    const int i = r / S, a = r % S;
    const unsigned r0 = noff[i], cnt = noff[i + 1] - r0;
    const int pos = find_col(ncols + r0, (int)cnt, (unsigned)i);
    dinv[r] = 1.0 / vals[(size_t)S * S * r0 + (size_t)a * S * cnt + (size_t)S * pos + a];
}

// r = b - r (r holds A x),  z = M^-1 r,  p = z;  partials of (z.r, b.b, r.r)      cg.rs:388-404
static __global__ void __launch_bounds__(256) k_cg_init(int n, const double* b, const double* dinv, double* r, double* z, double* p,
                                                 double* partial /* gridDim.x x 3 */) {
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const double ri = b[i] - r[i];
        const double zi = dinv ? dinv[i] * ri : ri;
        r[i] = ri;
        z[i] = zi;
        p[i] = zi;
        s[0] = fma(zi, ri, s[0]);
        s[1] = fma(b[i], b[i], s[1]);
        s[2] = fma(ri, ri, s[2]);
    }
    block_sum_store<3>(s, partial + 3 * blockIdx.x);
}

// x += alpha p,  r -= alpha Ap,  z = M^-1 r;  partials of (z.r, r.r)               cg.rs:453-468
static __global__ void __launch_bounds__(256) k_cg_update(int n, double alpha, const double* p, const double* Ap, const double* dinv,
                                                   double* x, double* r, double* z, double* partial /* gridDim.x x 2 */) {
    double s[2] = {0.0, 0.0};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        x[i] += alpha * p[i];
        const double ri = r[i] - alpha * Ap[i];
        const double zi = dinv ? dinv[i] * ri : ri;
        r[i] = ri;
        z[i] = zi;
        s[0] = fma(zi, ri, s[0]);
        s[1] = fma(ri, ri, s[1]);
    }
    block_sum_store<2>(s, partial + 2 * blockIdx.x);
}

// p = beta p + z                                                                   cg.rs:470-474
static __global__ void __launch_bounds__(256) k_cg_direction(int n, double beta, const double* z, double* p) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = beta * p[i] + z[i];
}

// ---- error integrals (src/error.rs:287-372): one lane per (element, quadrature point)
//   WHICH 0:  w |det J| |u_h(x_q) - u(x_q)|^2                      make_L2_error_squared_integrand   :222-236
//   WHICH 1:  w |det J| |grad u_h(x_q) - grad u(x_q)|_F^2          make_H1_seminorm_error_squared_integrand :238-254
// exact[] holds the reference solution sampled by the caller at the physical points:  (E, nq, S) values, or
// (E, nq, D, S) gradients with grad[i][k] = d u_k / d x_i (OMatrix<GeometryDim, SolutionDim>).
template <int D, int S, int WHICH>
__global__ void __launch_bounds__(256) k_error_squared(const KArgs a, const SourceArgs sa, const double* uh, const double* exact,
                                                       double* partial) {
    double s[1] = {0.0};
    const long long total = a.num_elements * a.nq;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long e = i / a.nq;
        const int q = (int)(i % a.nq);
        const int* nodes = a.conn + (size_t)e * sa.N;
        double J[D][D];
#pragma unroll
        for (int r = 0; r < D; ++r)
#pragma unroll
            for (int c = 0; c < D; ++c) J[r][c] = 0.0;
        for (int g = 0; g < sa.NG; ++g) {
            const double* v = a.verts + (size_t)nodes[g] * D;
            const double* gg = a.ggeom + ((size_t)q * sa.NG + g) * D;
#pragma unroll
            for (int r = 0; r < D; ++r)
#pragma unroll
                for (int c = 0; c < D; ++c) J[r][c] = fma(v[r], gg[c], J[r][c]);
        }
        const double detJ = det_small<D>(J);
        double err2 = 0.0;
        if (WHICH == 0) {
            double u[S];
#pragma unroll
            for (int k = 0; k < S; ++k) u[k] = 0.0;
            for (int n = 0; n < sa.N; ++n) {
                const double ph = a.phiref[(size_t)q * sa.N + n];
#pragma unroll
                for (int k = 0; k < S; ++k) u[k] = fma(ph, uh[(size_t)nodes[n] * S + k], u[k]);
            }
#pragma unroll
            for (int k = 0; k < S; ++k) {
                const double d = u[k] - exact[(size_t)i * S + k];
                err2 = fma(d, d, err2);
            }
        } else {
            double Ji[D][D];
            if (detJ == 0.0) {
                report_singular(a.status, e);
                continue;
            }
            inv_small(J, detJ, Ji);
            double gu[D][S];
#pragma unroll
            for (int r = 0; r < D; ++r)
#pragma unroll
                for (int k = 0; k < S; ++k) gu[r][k] = 0.0;
            for (int n = 0; n < sa.N; ++n) {
                const double* gr = a.gref + ((size_t)q * sa.N + n) * D;
                double g[D];
#pragma unroll
                for (int r = 0; r < D; ++r) {
                    double t = 0.0;
#pragma unroll
                    for (int c = 0; c < D; ++c) t = fma(Ji[c][r], gr[c], t);  // J^-T grad_ref
                    g[r] = t;
                }
#pragma unroll
                for (int r = 0; r < D; ++r)
#pragma unroll
                    for (int k = 0; k < S; ++k) gu[r][k] = fma(g[r], uh[(size_t)nodes[n] * S + k], gu[r][k]);
            }
#pragma unroll
            for (int r = 0; r < D; ++r)
#pragma unroll
                for (int k = 0; k < S; ++k) {
                    const double d = gu[r][k] - exact[((size_t)i * D + r) * S + k];
                    err2 = fma(d, d, err2);
                }
        }
        s[0] = fma(a.qw[q] * fabs(detJ), err2, s[0]);
    }
    block_sum_store<1>(s, partial + blockIdx.x);
}

// ---- matrix-free operator (engine_vector.hip): the generic parts; the tiles' passes are in vector_tiles.hip

// d = 1 / d (the matrix-free Jacobi preconditioner)
static __global__ void __launch_bounds__(256) k_reciprocal(int n, double* d) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) d[i] = 1.0 / d[i];
}

// |x|_inf over the entries the element pass sees (those of Dirichlet nodes excluded; dmask may be null) as the bits of a non-negative
// double (an integer maximum: order-free); *bits must be zero on entry
static __global__ void __launch_bounds__(256) k_mf_absmax(int n, int S, const double* x, const unsigned char* dmask, unsigned long long* bits) {
    __shared__ unsigned long long red[256];
    unsigned long long m = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        if (!dof_fixed_at(dmask, i, S)) m = max(m, (unsigned long long)__double_as_longlong(fabs(x[i])));
    red[threadIdx.x] = m;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = max(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax(bits, red[0]);
}

// the operand of the element pass: x 2^-e (mf_exponent), the entries of the Dirichlet nodes (dmask may be null) zeroed so that their columns vanish
static __global__ void __launch_bounds__(256) k_mf_operand(int n, int S, const double* x, const unsigned char* dmask, const unsigned long long* bits,
                                                           double* xm) {
    const int e = mf_exponent(bits);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        xm[i] = dof_fixed_at(dmask, i, S) ? 0.0 : ldexp(x[i], -e);
}

// node sums times 2^e (mf_exponent), rows of the Dirichlet nodes = scale x (dmask may be null), and the per-workgroup partials of x . y (dot_partial may be null)
static __global__ void __launch_bounds__(256) k_mf_finish(int n, int S, const double* x, const unsigned char* dmask, const double* scale,
                                                          const unsigned long long* bits, double* y, double* dot_partial) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    double d[1] = {0.0};
    if (i < n) {
        const double yv = dof_fixed_at(dmask, i, S) ? *scale * x[i] : ldexp(y[i], mf_exponent(bits));
        y[i] = yv;
        d[0] = x[i] * yv;
    }
    if (dot_partial) block_sum_store<1>(d, dot_partial + blockIdx.x);
}

// the scale of the Dirichlet rows, as apply_homogeneous_dirichlet_bc_csr takes it (global.rs:379-451): |first nonzero diagonal entry| in row
// order, or 1.  First pass: the lowest row with a nonzero entry (an integer minimum: order-free); second: the scale
static __global__ void __launch_bounds__(256) k_mf_first_nonzero(int n, const double* diag, unsigned long long* first) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && diag[i] != 0.0) atomicMin(first, (unsigned long long)i);
}
static __global__ void k_mf_scale(const double* diag, const unsigned long long* first, double* scale) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *scale = *first == ~0ull ? 1.0 : fabs(diag[*first]);
}
static __global__ void __launch_bounds__(256) k_mf_dirichlet_diag(int n, int S, const unsigned char* dmask, const double* scale, double* diag) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && dof_fixed_at(dmask, i, S)) diag[i] = *scale;
}

// ---- the matrix-free map off the tiles (the kinds outside them: Hex27, Tet10, Quad9, Tri6, Hex20, Tet20; a mesh without tile tables):
// one thread per element, the tables walked at run time like k_error_squared, fe[a][e][c] for k_vector_from_elements_soa.
// Point q of element e: J from the geometry vertices, J^-1 and s = w |det J| (false: det J == 0, the caller reports it) ...
template <int D>
__device__ __forceinline__ bool mf_point(const KArgs& a, const int* nodes, int NG, int q, double (&Ji)[D][D], double& s) {
    double J[D][D];
#pragma unroll
    for (int r = 0; r < D; ++r)
#pragma unroll
        for (int c = 0; c < D; ++c) J[r][c] = 0.0;
    for (int g = 0; g < NG; ++g) {
        const double* v = a.verts + (size_t)nodes[g] * D;
        const double* gg = a.ggeom + ((size_t)q * NG + g) * D;
#pragma unroll
        for (int r = 0; r < D; ++r)
#pragma unroll
            for (int c = 0; c < D; ++c) J[r][c] = fma(v[r], gg[c], J[r][c]);
    }
    const double detJ = det_small<D>(J);
    if (detJ == 0.0) return false;
    inv_small(J, detJ, Ji);
    s = a.qw[q] * fabs(detJ);
    return true;
}
// ... and g_n = J^-T ghat_n, the physical gradient of basis function n there
template <int D>
__device__ __forceinline__ void mf_grad(const KArgs& a, int N, int q, int n, const double (&Ji)[D][D], double (&g)[D]) {
    physical_gradient<D>(Ji, a.gref + ((size_t)q * N + n) * D, g);
}

// y = T(u) x (= A x for FH_LAPLACE and FH_LINEAR_ELASTIC) for any element kind, deterministic: grad x = J^-T sum_n ghat_n x_n^T per point (and
// grad u from a.u, may be null: zero, for the nonlinear operators only), dP(F)[grad x^T] by tangent_lin / tangent_apply (material.hpp;
// for the linear operators the stress of material_point without F), element vectors f_n = w |det J| dP g_n by local node.  Inactive elements
// write zeros.  EX (the nonlinear operators; here and in the two kernels below): the per-element expansion of a.theta applied to grad u at
// the point, the result scaled (material.hpp, Stretch); EX = false is the kernel as it was.
template <int D, int S, int OP, bool EX = false>
__global__ void __launch_bounds__(256) k_mf_apply_elements(const KArgs a, int N, int NG, const unsigned char* active, const double* x, double* fe) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.num_elements) return;
    const bool live = !active || active[e] != 0;
    const int* nodes = a.conn + (size_t)e * N;
    auto out = [&](int n) { return fe + ((size_t)n * (size_t)a.num_elements + (size_t)e) * S; };
    for (int n = 0; n < N; ++n)
#pragma unroll
        for (int k = 0; k < S; ++k) out(n)[k] = 0.0;
    if (!live) return;
    const double* par_e = a.rule_map ? a.rparams + (size_t)a.rule_map[e] * a.nq * 2 : nullptr;
    for (int q = 0; q < a.nq; ++q) {
        double Ji[D][D], s;
        if (!mf_point<D>(a, nodes, NG, q, Ji, s)) {
            report_singular(a.status, e);
            continue;
        }
        double gu[D][S], gx[D][S];
#pragma unroll
        for (int r = 0; r < D; ++r)
#pragma unroll
            for (int k = 0; k < S; ++k) { gu[r][k] = 0.0; gx[r][k] = 0.0; }
        for (int n = 0; n < N; ++n) {
            double g[D];
            mf_grad<D>(a, N, q, n, Ji, g);
#pragma unroll
            for (int k = 0; k < S; ++k) {
                const double xv = x[(size_t)nodes[n] * S + k];
                double uv = 0.0;
                if constexpr (op_depends_on_u(OP)) uv = a.u ? a.u[(size_t)nodes[n] * S + k] : 0.0;
#pragma unroll
                for (int r = 0; r < D; ++r) {
                    if constexpr (op_depends_on_u(OP)) gu[r][k] = fma(g[r], uv, gu[r][k]);
                    gx[r][k] = fma(g[r], xv, gx[r][k]);
                }
            }
        }
        if constexpr (EX) {
            static_assert(!EX || op_depends_on_u(OP), "the tangent of a linear operator does not see the expansion");
            const Stretch<OP, D> st = element_stretch<OP, D>(a, e);
            stretch_strain<OP, D, S>(st, gu);
            s *= st.sT;
        }
        double mu, lambda;
        point_params<OP>(a, par_e, q, mu, lambda);
        TangentLin<OP, D> L;
        tangent_lin<OP, D, S>(gu, mu, lambda, L);
        double dP[S][D];
        tangent_apply<OP, D, S>(L, gx, dP);
        for (int n = 0; n < N; ++n) {
            double g[D];
            mf_grad<D>(a, N, q, n, Ji, g);
            double* o = out(n);
#pragma unroll
            for (int i = 0; i < S; ++i) {
                double t = 0.0;
#pragma unroll
                for (int r = 0; r < D; ++r) t = fma(dP[i][r], g[r], t);
                o[i] = fma(s, t, o[i]);
            }
        }
    }
}

// the residual r(u) of any element kind without atomics (the Newton residual off the tiles, engine_vector.hip): per point grad u = J^-T
// sum_n ghat_n u_n^T (a.u, may be null: zero), the stress P of material_point (material.hpp), element vectors f_n = w |det J| P g_n by local node into
// fe[a][e][c] for the ordered node sums of k_vector_from_elements_soa.  Inactive elements write zeros; det J == 0 is reported like the residual.
template <int D, int S, int OP, bool EX = false>
__global__ void __launch_bounds__(256) k_residual_elements(const KArgs a, int N, int NG, const unsigned char* active, double* fe) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.num_elements) return;
    const bool live = !active || active[e] != 0;
    const int* nodes = a.conn + (size_t)e * N;
    auto out = [&](int n) { return fe + ((size_t)n * (size_t)a.num_elements + (size_t)e) * S; };
    for (int n = 0; n < N; ++n)
#pragma unroll
        for (int k = 0; k < S; ++k) out(n)[k] = 0.0;
    if (!live) return;
    const double* par_e = a.rule_map ? a.rparams + (size_t)a.rule_map[e] * a.nq * 2 : nullptr;
    for (int q = 0; q < a.nq; ++q) {
        double Ji[D][D], s;
        if (!mf_point<D>(a, nodes, NG, q, Ji, s)) {
            report_singular(a.status, e);
            continue;
        }
        double gu[D][S];
#pragma unroll
        for (int r = 0; r < D; ++r)
#pragma unroll
            for (int k = 0; k < S; ++k) gu[r][k] = 0.0;
        if (a.u)
            for (int n = 0; n < N; ++n) {
                double g[D];
                mf_grad<D>(a, N, q, n, Ji, g);
#pragma unroll
                for (int k = 0; k < S; ++k) {
                    const double uv = a.u[(size_t)nodes[n] * S + k];
#pragma unroll
                    for (int r = 0; r < D; ++r) gu[r][k] = fma(g[r], uv, gu[r][k]);
                }
            }
        if constexpr (EX) {
            const Stretch<OP, D> st = element_stretch<OP, D>(a, e);
            stretch_strain<OP, D, S>(st, gu);
            s *= st.sP;
        }
        double mu, lambda;
        point_params<OP>(a, par_e, q, mu, lambda);
        double P[S][D], psi;
        material_point<OP, D, S, EP_VECTOR>(gu, mu, lambda, P, psi);
        for (int n = 0; n < N; ++n) {
            double g[D];
            mf_grad<D>(a, N, q, n, Ji, g);
            double* o = out(n);
#pragma unroll
            for (int i = 0; i < S; ++i) {
                double t = 0.0;
#pragma unroll
                for (int r = 0; r < D; ++r) t = fma(P[i][r], g[r], t);
                o[i] = fma(s, t, o[i]);
            }
        }
    }
}

// the diagonal of the same map: entry (n, k) = sum_q s (dP[e_k g_n^T] g_n)_k, in ascending q.  The linear operators in closed form, as
// diagonal_element_body (element_pass.hpp):  Laplace  s |g_n|^2,  LinearElastic  s (mu (|g_n|^2 + g_n,k^2) + lambda g_n,k^2); the nonlinear
// ones by tangent_apply on the unit directions, as tangent_diagonal_body.
template <int D, int S, int OP, bool EX = false>
__global__ void __launch_bounds__(256) k_mf_diagonal_elements(const KArgs a, int N, int NG, const unsigned char* active, double* fe) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.num_elements) return;
    const bool live = !active || active[e] != 0;
    const int* nodes = a.conn + (size_t)e * N;
    auto out = [&](int n) { return fe + ((size_t)n * (size_t)a.num_elements + (size_t)e) * S; };
    for (int n = 0; n < N; ++n)
#pragma unroll
        for (int k = 0; k < S; ++k) out(n)[k] = 0.0;
    if (!live) return;
    const double* par_e = a.rule_map ? a.rparams + (size_t)a.rule_map[e] * a.nq * 2 : nullptr;
    for (int q = 0; q < a.nq; ++q) {
        double Ji[D][D], s;
        if (!mf_point<D>(a, nodes, NG, q, Ji, s)) {
            report_singular(a.status, e);
            continue;
        }
        double gu[D][S];
#pragma unroll
        for (int r = 0; r < D; ++r)
#pragma unroll
            for (int k = 0; k < S; ++k) gu[r][k] = 0.0;
        if constexpr (op_depends_on_u(OP)) {
            for (int n = 0; n < N; ++n) {
                double g[D];
                mf_grad<D>(a, N, q, n, Ji, g);
#pragma unroll
                for (int k = 0; k < S; ++k) {
                    const double uv = a.u ? a.u[(size_t)nodes[n] * S + k] : 0.0;
#pragma unroll
                    for (int r = 0; r < D; ++r) gu[r][k] = fma(g[r], uv, gu[r][k]);
                }
            }
        }
        if constexpr (EX) {
            static_assert(!EX || op_depends_on_u(OP), "the diagonal of a linear operator does not see the expansion");
            const Stretch<OP, D> st = element_stretch<OP, D>(a, e);
            stretch_strain<OP, D, S>(st, gu);
            s *= st.sT;
        }
        double mu, lambda;
        point_params<OP>(a, par_e, q, mu, lambda);
        TangentLin<OP, D> L;
        tangent_lin<OP, D, S>(gu, mu, lambda, L);
        for (int n = 0; n < N; ++n) {
            double g[D], gsq = 0.0;
            mf_grad<D>(a, N, q, n, Ji, g);
#pragma unroll
            for (int r = 0; r < D; ++r) gsq = fma(g[r], g[r], gsq);
            double* o = out(n);
#pragma unroll
            for (int c = 0; c < S; ++c) {
                double t;
                if constexpr (OP == FH_LAPLACE) {
                    t = gsq;
                } else if constexpr (OP == FH_LINEAR_ELASTIC) {
                    t = mu * (gsq + g[c] * g[c]) + lambda * (g[c] * g[c]);
                } else {
                    double gx[D][S], dP[S][D];
#pragma unroll
                    for (int r = 0; r < D; ++r)
#pragma unroll
                        for (int k = 0; k < S; ++k) gx[r][k] = k == c ? g[r] : 0.0;
                    tangent_apply<OP, D, S>(L, gx, dP);
                    t = 0.0;
#pragma unroll
                    for (int r = 0; r < D; ++r) t = fma(dP[c][r], g[r], t);
                }
                o[c] = fma(s, t, o[c]);
            }
        }
    }
}


// ---- the mass term of the shifted map (alpha M + beta T(u)) x, engine_vector.hip (mass_element_body: element_pass.hpp).
// the mass term off the tiles (every kind, rule-set groups): one thread per element, fe[a][e][c] for k_vector_from_elements_soa; x null: the
// diagonal.  dmask (may be null): the entries of the Dirichlet nodes read as zero.  Inactive elements write zeros.
template <int D, int S, int N, int NG>
__global__ void __launch_bounds__(256) k_mass_elements(const KArgs a, const unsigned char* active, const double* rho, int rho_per_elem,
                                                       const double* x, const unsigned char* dmask, double* fe) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.num_elements) return;
    const int* nodes = a.conn + (size_t)e * N;
    auto out = [&](int n) { return fe + ((size_t)n * (size_t)a.num_elements + (size_t)e) * S; };
    for (int n = 0; n < N; ++n)
#pragma unroll
        for (int k = 0; k < S; ++k) out(n)[k] = 0.0;
    if (active && active[e] == 0) return;
    double X[NG][D];
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
        for (int r = 0; r < D; ++r) X[g][r] = a.verts[(size_t)nodes[g] * D + r];
    auto xv = [&](int n, int k) {
        const int nd = nodes[n];
        return dof_fixed(dmask, nd, k) ? 0.0 : x[(size_t)nd * S + k];
    };
    // (mass_element_body's arithmetic, accumulated in fe rather than in registers: f[27][3] does not fit beside the rest)
    const double r = rho[rho_per_elem ? e : 0];
    for (int q = 0; q < a.nq; ++q) {
        const double s = mass_point_weight<D, NG>(a, X, q) * r;
        const double* phi = a.phiref + (size_t)q * N;
        if (!x) {
            for (int n = 0; n < N; ++n) {
                const double t = s * phi[n] * phi[n];
#pragma unroll
                for (int k = 0; k < S; ++k) out(n)[k] += t;
            }
            continue;
        }
        double xq[S];
#pragma unroll
        for (int k = 0; k < S; ++k) xq[k] = 0.0;
        for (int n = 0; n < N; ++n)
#pragma unroll
            for (int k = 0; k < S; ++k) xq[k] = fma(phi[n], xv(n, k), xq[k]);
        for (int n = 0; n < N; ++n) {
            const double t = s * phi[n];
            double* o = out(n);
#pragma unroll
            for (int k = 0; k < S; ++k) o[k] = fma(t, xq[k], o[k]);
        }
    }
}

// y = alpha m + beta t (m, t: may be null = zero; t may be y), rows of the Dirichlet nodes = scale x (dmask may be null), and the
// per-workgroup partials of x . y (dot_partial may be null; x may be null without dmask and dot_partial: the diagonal)
static __global__ void __launch_bounds__(256) k_mf_shift_combine(int n, int S, double alpha, const double* m, double beta, const double* t,
                                                                 const double* x, const unsigned char* dmask, const double* scale, double* y,
                                                                 double* dot_partial) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    double d[1] = {0.0};
    if (i < n) {
        const double v = m ? alpha * m[i] : 0.0;
        const double yv = dof_fixed_at(dmask, i, S) ? *scale * x[i] : (t ? fma(beta, t[i], v) : v);
        y[i] = yv;
        if (dot_partial) d[0] = x[i] * yv;
    }
    if (dot_partial) block_sum_store<1>(d, dot_partial + blockIdx.x);
}

// the Newton residual off the tiles (engine_newton.hip): F = alpha m + beta (r - f) (m null: alpha = 0; f null: zero) with the rows of the
// Dirichlet nodes (dmask, may be null) zero, and the per-workgroup partials of |F|^2 -- the same arithmetic as k_newton_from_partials
static __global__ void __launch_bounds__(256) k_newton_combine(int n, int S, double alpha, const double* m, double beta, const double* r,
                                                               const double* f, const unsigned char* dmask, double* F, double* norm_partial) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    double sq[1] = {0.0};
    if (i < n) {
        const double rf = f ? r[i] - f[i] : r[i];
        const double v = dof_fixed_at(dmask, i, S) ? 0.0 : (m ? fma(beta, rf, alpha * m[i]) : beta * rf);
        F[i] = v;
        sq[0] = v * v;
    }
    block_sum_store<1>(sq, norm_partial + blockIdx.x);
}

// the line-search move of the Newton solve, in place on the context's u: u += da p with p = -q (q: the PCG solution of J q = F; null: no
// move), and d = u - u_ref (u_ref null: zero) in the same sweep when d is given (the operand of the next mass term)
static __global__ void __launch_bounds__(256) k_newton_move(int n, double da, const double* q, double* u, const double* u_ref, double* d) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double v = u[i];
    if (q) {
        v = fma(da, -q[i], v);
        u[i] = v;
    }
    if (d) d[i] = u_ref ? v - u_ref[i] : v;
}

}  // namespace fenris_hip
