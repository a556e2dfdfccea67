#pragma once
// Uniform refinement kernels (engine_hierarchy.hip): what the refinement adds to the labelling of
// hierarchy_kernels.hpp.  A refinement labels the new points of every cell (the candidates; the old vertices keep their indices, and
// every new point goes through the sort: s0 = nv, Sm = S, keep) and then writes children, where an elevation writes one high cell.
//
// Tri3: the children [0,3,5] [3,1,4] [5,4,2] [3,4,5] are the reference's [a,d,f] [d,b,e] [f,e,c] [d,e,f] (src/mesh/refinement/detail.rs:
// 116-127).  Only the vertex LABELS differ from the reference's: it labels the old vertices by first appearance too, here they keep
// their indices.
#include <hip/hip_runtime.h>

#include "hierarchy_kernels.hpp"

namespace fenris_hip {

// The children of a cell kind, by value in the kernel arguments.  Local index n + p names new point p: the table's local node.
struct RefineChildren {
    int n, P, C;                  // nodes per cell, new points per cell, children per cell
    signed char child[8][8];      // child k, node a: local index
};

// Stage 5a: the fine index of every candidate: N + the rank of its winner
__global__ void k_refine_fine_index(unsigned nocc, unsigned N, const unsigned* __restrict__ first, const unsigned long long* __restrict__ scan,
                                    unsigned* __restrict__ fine) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nocc) return;
    fine[i] = N + (unsigned)(scan[first[i]] >> LABEL_SHIFT);
}

// Stage 5b: the children.  One thread per node of a child: consecutive threads write consecutive words.
__global__ void k_refine_children(const int* __restrict__ conn, RefineChildren t, unsigned long long total, const unsigned* __restrict__ fine,
                                  unsigned long long* __restrict__ out) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const unsigned per_cell = (unsigned)(t.C * t.n);
    const unsigned long long cell = i / per_cell;
    const unsigned slot = (unsigned)(i % per_cell);
    const int l = t.child[slot / (unsigned)t.n][slot % (unsigned)t.n];
    out[i] = l < t.n ? (unsigned long long)conn[cell * t.n + l] : (unsigned long long)fine[cell * t.P + (l - t.n)];
}

// Stage 5c, coarse part: k_refine_coarse_rows (hierarchy_kernels.hpp)

// Stage 5c, new part: every winner writes its vertex and its transfer row.  Kept apart from k_elevate_rows on purpose: the position is
// the sum of the parents in ascending GLOBAL index times 1 / count -- the operations and their order of refine_hex8_uniform
// (host_inputs.cpp), so the bits are the host's: the sum starts at 0.0, the product is a product alone (nothing to contract it with),
// and 1 / count is exact.  The elevation follows the host converters instead, which sum in the cell's local node order.
template <int MP, int D>
__global__ void k_refine_new_rows(const double* __restrict__ verts, const int* __restrict__ conn, LabelTable t, unsigned nocc, unsigned N,
                                  const unsigned* __restrict__ first, const unsigned long long* __restrict__ scan, double* __restrict__ out_v,
                                  unsigned long long* __restrict__ off, unsigned long long* __restrict__ idx, double* __restrict__ w) {
#pragma clang fp contract(off)
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nocc || first[i] != i) return;
    unsigned k[MP];
    label_sorted_tuple<MP>(conn, t, i, k);
    const int cnt = t.t.cnt[(unsigned)t.s0 + i % (unsigned)t.S];
    const double wt = cnt == 2 ? 0.5 : cnt == 4 ? 0.25 : 0.125;
    const unsigned long long s = scan[i];
    const size_t v = (size_t)N + (size_t)(s >> LABEL_SHIFT);
    const unsigned long long pos = (unsigned long long)N + (s & ((1ull << LABEL_SHIFT) - 1));
    off[v] = pos;
#pragma unroll
    for (int r = 0; r < D; ++r) {
        double sum = 0.0;
#pragma unroll
        for (int q = 0; q < MP; ++q)
            if (q < cnt) sum += verts[(size_t)k[q] * D + r];
        out_v[v * D + r] = sum * wt;
    }
#pragma unroll
    for (int q = 0; q < MP; ++q)
        if (q < cnt) {
            idx[pos + q] = k[q];
            w[pos + q] = wt;
        }
}

}  // namespace fenris_hip
