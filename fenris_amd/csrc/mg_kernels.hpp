#pragma once
// Kernels of the geometric multigrid V-cycle (engine_mg.hip).  Every sum has a fixed order and none uses atomics, so a V-cycle repeats bit
// for bit.  Vectors are node-major with S components per node; the transfer tables are CSR by node and shared by the S components.
#include <hip/hip_runtime.h>

#include "device_common.hpp"

namespace fenris_hip_mg {

// xf += P xc on the fine dofs that are not Dirichlet (the correction is zero there): at most 8 parents per fine node, in table order
static __global__ void __launch_bounds__(256) k_mg_prolongate_add(int nf, int S, const unsigned* p_off, const unsigned* p_idx, const double* p_w,
                                                           const unsigned char* dmask_f, const double* xc, double* xf) {
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < nf * S; t += gridDim.x * blockDim.x) {
        const int i = t / S, s = t - i * S;
        if (fenris_hip::dof_fixed(dmask_f, i, s)) continue;
        double acc = 0.0;
        for (unsigned k = p_off[i]; k < p_off[i + 1]; ++k) acc = fma(p_w[k], xc[(size_t)S * p_idx[k] + s], acc);
        xf[t] += acc;
    }
}

// bc = P^T (b - Ax) per coarse dof, gathered over the transpose table in its fixed (ascending fine index) order.  The fine Dirichlet dofs
// contribute nothing and the coarse Dirichlet rows are zero, so that restriction and prolongation stay transposes of each other.
static __global__ void __launch_bounds__(256) k_mg_restrict_residual(int nc, int S, const unsigned* r_off, const unsigned* r_idx, const double* r_w,
                                                              const unsigned char* dmask_f, const unsigned char* dmask_c, const double* b,
                                                              const double* Ax, double* bc) {
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < nc * S; t += gridDim.x * blockDim.x) {
        const int j = t / S, s = t - j * S;
        double acc = 0.0;
        if (!fenris_hip::dof_fixed(dmask_c, j, s))
            for (unsigned k = r_off[j]; k < r_off[j + 1]; ++k) {
                const unsigned i = r_idx[k];
                if (fenris_hip::dof_fixed(dmask_f, i, s)) continue;
                const size_t f = (size_t)S * i + s;
                acc = fma(r_w[k], b[f] - Ax[f], acc);
            }
        bc[t] = acc;
    }
}

// start of the Chebyshev smoother: r = b - Ax (Ax null: x = 0, r = b, and x is zeroed), d = D^-1 r / theta
static __global__ void __launch_bounds__(256) k_mg_cheb_start(int n, const double* b, const double* Ax, const double* diag, double inv_theta, double* x,
                                                       double* r, double* d) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const double ri = Ax ? b[i] - Ax[i] : b[i];
        if (!Ax) x[i] = 0.0;
        r[i] = ri;
        d[i] = ri / diag[i] * inv_theta;
    }
}

// one inner step: x += d;  r -= A d;  d = c1 d + c2 D^-1 r   (c1 = rho' rho, c2 = 2 rho' / delta)
static __global__ void __launch_bounds__(256) k_mg_cheb_step(int n, const double* Ad, const double* diag, double c1, double c2, double* x, double* r,
                                                      double* d) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const double di = d[i];
        x[i] += di;
        const double ri = r[i] - Ad[i];
        r[i] = ri;
        d[i] = c1 * di + c2 * (ri / diag[i]);
    }
}

// the last step x += d
static __global__ void __launch_bounds__(256) k_mg_add(int n, const double* d, double* x) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) x[i] += d[i];
}

// the Dirichlet rows of a V-cycle's result: x = b / D there (D = the scale of the rows)
static __global__ void __launch_bounds__(256) k_mg_dirichlet_rows(int n, int S, const unsigned char* dmask, const double* b, const double* diag, double* x) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        if (fenris_hip::dof_fixed_at(dmask, i, S)) x[i] = b[i] / diag[i];
}

// uc = the fine values at each coarse node's injected fine copy
static __global__ void __launch_bounds__(256) k_mg_inject(int nc, int S, const unsigned* inj, const double* uf, double* uc) {
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < nc * S; t += gridDim.x * blockDim.x) {
        const int j = t / S, s = t - j * S;
        uc[t] = uf[(size_t)S * inj[j] + s];
    }
}

// x = Ainv b on the coarsest level: one wavefront per row, lane l sums the columns l, l + 64, ... in order, then a fixed butterfly
static __global__ void __launch_bounds__(256) k_mg_dense_apply(int n, const double* Ainv, const double* b, double* x) {
    const int lane = threadIdx.x & 63;
    for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += gridDim.x * 4) {
        const double* a = Ainv + (size_t)row * n;
        double acc = 0.0;
        for (int j = lane; j < n; j += 64) acc = fma(a[j], b[j], acc);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) x[row] = acc;
    }
}

// the start vector of the eigenvalue estimate: a fixed hash of the index in [-1, 1), zero on the Dirichlet dofs
static __global__ void __launch_bounds__(256) k_mg_start_vector(int n, int S, const unsigned char* dmask, double* v) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        unsigned long long h = (unsigned long long)i * 0x9e3779b97f4a7c15ull + 0x632be59bd9b4e019ull;
        h ^= h >> 31;
        h *= 0xbf58476d1ce4e5b9ull;
        h ^= h >> 29;
        const double u = (double)(h >> 11) * 0x1p-53;
        v[i] = fenris_hip::dof_fixed_at(dmask, i, S) ? 0.0 : 2.0 * u - 1.0;
    }
}

// PCG with the V-cycle as preconditioner (engine_solver.hip): x += alpha p, r -= alpha Ap and the partials of r . r into slot 1 of 2
static __global__ void __launch_bounds__(256) k_mg_cg_update(int n, double alpha, const double* p, const double* Ap, double* x, double* r,
                                                      double* partial /* gridDim.x x 2 */) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        x[i] += alpha * p[i];
        const double ri = r[i] - alpha * Ap[i];
        r[i] = ri;
        s = fma(ri, ri, s);
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[2 * blockIdx.x + 1] = red[0];
}

// the partials of z . r into slot 0 of K; p = z when p is given (the first direction)
static __global__ void __launch_bounds__(256) k_mg_cg_zr(int n, int K, const double* z, const double* r, double* p, double* partial) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const double zi = z[i];
        if (p) p[i] = zi;
        s = fma(zi, r[i], s);
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[(size_t)K * blockIdx.x] = red[0];
}

}  // namespace fenris_hip_mg
