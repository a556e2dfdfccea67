// Block-vector kernels of the LOBPCG eigensolver (engine_eigs.hip): tall-skinny Gram matrices G = S^T T, block recombination Y = S C and
// block residuals R_j = (K X)_j - theta_j (M X)_j with their column norms.  A block vector is column-major: column j is a contiguous
// n-vector at base + j ld (ld >= n), so every column can be handed to the matrix-free maps as it is; n < 2^31 as in the CG path.  The
// columns of an operand may come from up to three such blocks with a common ld ([X W P] without copying them together): BlockCols.
// No floating-point atomics: every reduction leaves per-workgroup partials that are summed in workgroup order, so results repeat bit for
// bit.  Rows between n and ld are never read or written.
#pragma once
#include <hip/hip_runtime.h>

#include "solver_kernels.hpp"

namespace fenris_hip {

constexpr int BLOCK_MAX_COLS = 96;      // three blocks of FH_EIG_MAX_BLOCK
constexpr int BLOCK_GRAM_ROWS = 32;     // rows of a chunk staged in LDS by k_block_gram
constexpr int BLOCK_COMBINE_MAX_Q = 64; // output columns of one k_block_combine launch (both outputs together)

// the columns of an operand: c[0] columns at p[0], then c[1] at p[1], then c[2] at p[2]; column k of a part is at p + k ld
struct BlockCols {
    const double* p[3];
    int c[3];
    long long ld;
    __host__ __device__ int total() const { return c[0] + c[1] + c[2]; }
    __device__ __forceinline__ const double* col(int j) const {
        if (j < c[0]) return p[0] + (long long)j * ld;
        j -= c[0];
        if (j < c[1]) return p[1] + (long long)j * ld;
        j -= c[1];
        return p[2] + (long long)j * ld;
    }
};
struct BlockScalars { double v[32]; };   // one double per column of a block of at most FH_EIG_MAX_BLOCK (passed by value)
struct BlockIndex { int v[32]; };        // one column index per column

// ---- G = S^T T, S n x p, T n x q, p <= 16 A, q <= 16 A.  Workgroup b owns the rows [b per, (b + 1) per) and walks them in chunks of
// BLOCK_GRAM_ROWS rows: the chunk of S and of T is staged in LDS row by row (row stride 16 A + 1 doubles: the stores of a wavefront, one
// row per lane, then hit different banks), the columns past p and q hold zeros.  The 256 threads form a 16 x 16 grid; thread (ti, tj) owns
// the A x A entries (ti A + a, tj + 16 b): its S operands are A neighbouring doubles shared by the 16 threads of a ti (a broadcast), its T
// operands are 16 neighbouring doubles over tj (no bank conflict).  A x A accumulators in registers (A = 6: 72 VGPRs), no scratch.
// LDS: 2 * 32 * (16 A + 1) * 8 bytes (A = 6: 49664, three workgroups per CU).  Rows of Dirichlet nodes (mask[(int)row / sdim]) count as zero.
// The partial tile of workgroup b goes to partial + b p q (row-major p x q); k_block_gram_sum adds them in workgroup order.
template <int A>
__global__ void __launch_bounds__(256) k_block_gram(int n, int per, BlockCols S, BlockCols T, const unsigned char* mask, int sdim, double* partial) {
    constexpr int LD = 16 * A + 1, R = BLOCK_GRAM_ROWS;
    __shared__ double sS[R * LD];
    __shared__ double sT[R * LD];
    const int p = S.total(), q = T.total();
    const int tid = threadIdx.x, ti = tid >> 4, tj = tid & 15;
    for (int e = tid; e < R * LD; e += 256) { sS[e] = 0.0; sT[e] = 0.0; }
    double acc[A][A];
#pragma unroll
    for (int a = 0; a < A; ++a)
#pragma unroll
        for (int b = 0; b < A; ++b) acc[a][b] = 0.0;
    const long long lo = (long long)blockIdx.x * per;
    const long long hi = lo + per < (long long)n ? lo + per : (long long)n;
    for (long long r0 = lo; r0 < hi; r0 += R) {
        __syncthreads();   // (the zero fill, or the previous chunk's reads)
        for (int e = tid; e < R * p; e += 256) {
            const int r = e % R, k = e / R;
            const long long row = r0 + r;
            double v = 0.0;
            if (row < hi && !dof_fixed_at(mask, (int)row, sdim)) v = S.col(k)[row];
            sS[r * LD + k] = v;
        }
        for (int e = tid; e < R * q; e += 256) {
            const int r = e % R, k = e / R;
            const long long row = r0 + r;
            double v = 0.0;
            if (row < hi && !dof_fixed_at(mask, (int)row, sdim)) v = T.col(k)[row];
            sT[r * LD + k] = v;
        }
        __syncthreads();
#pragma unroll 4
        for (int r = 0; r < R; ++r) {
            double s[A], t[A];
#pragma unroll
            for (int a = 0; a < A; ++a) s[a] = sS[r * LD + ti * A + a];
#pragma unroll
            for (int b = 0; b < A; ++b) t[b] = sT[r * LD + tj + 16 * b];
#pragma unroll
            for (int a = 0; a < A; ++a)
#pragma unroll
                for (int b = 0; b < A; ++b) acc[a][b] = fma(s[a], t[b], acc[a][b]);
        }
    }
    double* out = partial + (size_t)blockIdx.x * p * q;
#pragma unroll
    for (int a = 0; a < A; ++a)
#pragma unroll
        for (int b = 0; b < A; ++b) {
            const int i = ti * A + a, j = tj + 16 * b;
            if (i < p && j < q) out[i * q + j] = acc[a][b];
        }
}

// out[e] = sum over the workgroups b, in order, of partial[b count + e]
static __global__ void __launch_bounds__(256) k_block_gram_sum(int count, int blocks, const double* partial, double* out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= count) return;
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += partial[(size_t)b * count + e];
    out[e] = s;
}

// ---- Y1 = S C1 (+ Y1) and, from the same read of S, Y2 = S C2 (+ Y2): S n x p, C = [C1 C2] p x (q1 + q2) with q1 + q2 <= Q.  C is staged
// in LDS once per workgroup, row-major with row stride Q and zeros past q1 + q2 (p Q doubles: at most 96 * 64 * 8 = 49152 bytes); every
// thread owns a row at a time (a grid-stride loop over the rows), reads each column of S once (coalesced over the lanes) and keeps the Q
// sums of its row in registers (Q = 64: 128 VGPRs), the C operands being the same address for every lane (an LDS broadcast).  Neither Y may
// overlap S.  Rows >= n are not touched.
template <int Q>
__global__ void __launch_bounds__(256) k_block_combine(int n, BlockCols S, const double* C, int q1, double* Y1, int q2, double* Y2, long long ldy,
                                                       int accumulate) {
    extern __shared__ double sC[];
    const int p = S.total(), qt = q1 + q2;
    for (int e = threadIdx.x; e < p * Q; e += 256) {
        const int k = e / Q, j = e % Q;
        sC[e] = j < qt ? C[k * qt + j] : 0.0;
    }
    __syncthreads();
    for (long long row = (long long)blockIdx.x * 256 + threadIdx.x; row < n; row += (long long)gridDim.x * 256) {
        double acc[Q];   // (accumulating: the sums start from Y, so that a row of Y + S C is one inner product of p + 1 terms)
#pragma unroll
        for (int j = 0; j < Q; ++j) {
            acc[j] = 0.0;
            if (accumulate && j < q1) acc[j] = Y1[(long long)j * ldy + row];
            else if (accumulate && j < qt) acc[j] = Y2[(long long)(j - q1) * ldy + row];
        }
        int k = 0;
#pragma unroll
        for (int part = 0; part < 3; ++part) {
            const double* col = S.p[part] + row;
            for (int kk = 0; kk < S.c[part]; ++kk, ++k, col += S.ld) {
                const double s = *col;
                const double* cr = sC + k * Q;
#pragma unroll
                for (int j = 0; j < Q; ++j) acc[j] = fma(s, cr[j], acc[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < Q; ++j) {
            if (j < q1) Y1[(long long)j * ldy + row] = acc[j];
            else if (j < qt) Y2[(long long)(j - q1) * ldy + row] = acc[j];
        }
    }
}

// ---- R_j = (K X)_j - theta_j (M X)_j, zero on the rows of Dirichlet nodes; blockIdx.y is the column.  Workgroup (b, j) leaves the partials
// of |R_j|^2, |(M X)_j|^2, |(K X)_j|^2 over its rows at partial + 3 (j gridDim.x + b); k_block_norm_sum adds them in workgroup order.
static __global__ void __launch_bounds__(256) k_block_residual(int n, const double* KX, const double* MX, long long ld, BlockScalars theta,
                                                               const unsigned char* mask, int sdim, double* R, double* partial) {
    const int j = blockIdx.y;
    const double th = theta.v[j];
    const double* kx = KX + (long long)j * ld;
    const double* mx = MX + (long long)j * ld;
    double* r = R + (long long)j * ld;
    double s[3] = {0.0, 0.0, 0.0};
    for (long long row = (long long)blockIdx.x * 256 + threadIdx.x; row < n; row += (long long)gridDim.x * 256) {
        double a = kx[row], b = mx[row];
        if (dof_fixed_at(mask, (int)row, sdim)) { a = 0.0; b = 0.0; }
        const double v = fma(-th, b, a);
        r[row] = v;
        s[0] = fma(v, v, s[0]);
        s[1] = fma(b, b, s[1]);
        s[2] = fma(a, a, s[2]);
    }
    block_sum_store<3>(s, partial + 3 * ((size_t)j * gridDim.x + blockIdx.x));
}
// out[3 j + k] = sum over b, in order, of partial[3 (j blocks + b) + k]; one thread per (j, k)
static __global__ void __launch_bounds__(256) k_block_norm_sum(int cols, int blocks, const double* partial, double* out) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= 3 * cols) return;
    const int j = e / 3, k = e % 3;
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += partial[3 * ((size_t)j * blocks + b) + k];
    out[e] = s;
}

// ---- the start block: X(row, j) = u(row, j) in [-1, 1) off the Dirichlet rows, 0 on them, with
//   u(row, j) = (splitmix64((j << 32) | row) >> 11) 2^-52 - 1,
//   splitmix64(z): z += 0x9e3779b97f4a7c15; z = (z ^ z >> 30) 0xbf58476d1ce4e5b9; z = (z ^ z >> 27) 0x94d049bb133111eb; z ^ z >> 31
__device__ __forceinline__ double block_hash_unit(unsigned long long row, unsigned long long j) {
    unsigned long long z = ((j << 32) | row) + 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    return (double)(z >> 11) * 0x1p-52 - 1.0;
}
static __global__ void __launch_bounds__(256) k_block_fill(int n, long long ld, const unsigned char* mask, int sdim, double* X) {
    const int j = blockIdx.y;
    for (long long row = (long long)blockIdx.x * 256 + threadIdx.x; row < n; row += (long long)gridDim.x * 256)
        X[(long long)j * ld + row] = dof_fixed_at(mask, (int)row, sdim) ? 0.0 : block_hash_unit((unsigned long long)row, (unsigned long long)j);
}
// zero on the rows of Dirichlet nodes
static __global__ void __launch_bounds__(256) k_block_mask(int n, long long ld, const unsigned char* mask, int sdim, double* X) {
    const int j = blockIdx.y;
    for (long long row = (long long)blockIdx.x * 256 + threadIdx.x; row < n; row += (long long)gridDim.x * 256)
        if (dof_fixed_at(mask, (int)row, sdim)) X[(long long)j * ld + row] = 0.0;
}
// W_a = dinv . R_{idx[a]} off the Dirichlet rows, 0 on them (the Jacobi preconditioner on the active columns)
static __global__ void __launch_bounds__(256) k_block_jacobi(int n, long long ld, const double* dinv, const double* R, BlockIndex idx,
                                                             const unsigned char* mask, int sdim, double* W) {
    const int a = blockIdx.y;
    const double* r = R + (long long)idx.v[a] * ld;
    double* w = W + (long long)a * ld;
    for (long long row = (long long)blockIdx.x * 256 + threadIdx.x; row < n; row += (long long)gridDim.x * 256)
        w[row] = dof_fixed_at(mask, (int)row, sdim) ? 0.0 : dinv[row] * r[row];
}

}  // namespace fenris_hip
