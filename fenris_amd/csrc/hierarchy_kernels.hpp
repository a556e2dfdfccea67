#pragma once
// What the mesh hierarchy passes share (refine_kernels.hpp, coarsen_kernels.hpp, elevate_kernels.hpp): the parent table of a quadratic
// kind, the sorted parent tuple of a node, and the rows of vertices that keep their indices.  Templates and inline functions only: the
// header is included by several translation units.
#include <hip/hip_runtime.h>

namespace fenris_hip {

constexpr int COARSEN_MAX_NODES = 27;

// The parents of every local node of a cell kind, by value in the kernel arguments.
struct CoarsenTable {
    int n, nv;                                   // nodes per cell; vertex slots per cell (the first nv local nodes)
    signed char cnt[COARSEN_MAX_NODES];          // parents of local node l: 1 (a vertex slot: itself), 2, 4 or 8
    signed char par[COARSEN_MAX_NODES][8];       // ... as local nodes < nv
};

// the table of a quadratic kind and its linear kind; false for a kind without one (engine_coarsen.hip)
bool coarsen_table(int kind, CoarsenTable& t, int& linear_kind);

constexpr unsigned COARSEN_NONE = 0xFFFFFFFFu;   // padding of a tuple, and "no node" in the status words

// the nodes ec[par[0 .. cnt)] of one cell, ascending, padded with COARSEN_NONE (which sorts last: the number of parents is part of the
// tuple).  Odd-even transposition with compile-time indices: the tuple stays in registers.
template <int MP>
__device__ __forceinline__ void sorted_parent_tuple(const int* __restrict__ ec, const signed char* par, int cnt, unsigned (&k)[MP]) {
#pragma unroll
    for (int a = 0; a < MP; ++a) k[a] = a < cnt ? (unsigned)ec[par[a]] : COARSEN_NONE;
#pragma unroll
    for (int pass = 0; pass < MP; ++pass) {
#pragma unroll
        for (int i = pass & 1; i + 1 < MP; i += 2) {
            const unsigned lo = min(k[i], k[i + 1]), hi = max(k[i], k[i + 1]);
            k[i] = lo;
            k[i + 1] = hi;
        }
    }
}

// The vertices that keep their indices (the coarse ones of a refinement, stage 5c; the old ones under Tri6 and Quad9): positions copied,
// transfer rows the identity.  Thread N closes the offsets.
template <int D>
__global__ void k_refine_coarse_rows(const double* __restrict__ verts, unsigned N, unsigned long long num_fine, unsigned long long nnz,
                                     double* __restrict__ out_v, unsigned long long* __restrict__ off, unsigned long long* __restrict__ idx,
                                     double* __restrict__ w) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == N) off[num_fine] = nnz;
    if (i >= N) return;
#pragma unroll
    for (int r = 0; r < D; ++r) out_v[(size_t)i * D + r] = verts[(size_t)i * D + r];
    off[i] = i;
    idx[i] = i;
    w[i] = 1.0;
}

}  // namespace fenris_hip
