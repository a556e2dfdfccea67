#pragma once
// Degree elevation kernels (engine_hierarchy.hip): the quadratic mesh over a linear one and the transfer from
// the linear vertices to all of its nodes, numbered as the sequential sweeps fh_refine_to_quadratic and fh_hex8_to_hex27 number them
// (host_inputs.cpp): what the elevation adds to the labelling of hierarchy_kernels.hpp.
//
// Tet10, Hex20 and Hex27 label every slot (s0 = 0: the old vertex indices are not kept); Tri6 and Quad9 keep the old vertices and label
// the other slots (s0 = nv, keep).  The centre of a Quad9 or Hex27 is the last slot of its cell and is not matched (Sm = S - 1).  A
// winner computes its position from its own cell in its local node order.
#include <hip/hip_runtime.h>

#include "hierarchy_kernels.hpp"   // LabelTable: the parents of every local node of the high kind; sorted_parent_tuple; k_refine_coarse_rows

namespace fenris_hip {

// Stage 5a: the high cells.  One thread per node of a cell: consecutive threads write consecutive words.  A labelled slot reads the rank
// of its winner; `base` is the number of kept vertices (0 where none is kept).
__global__ void k_elevate_cells(const int* __restrict__ conn, LabelTable t, unsigned long long total, unsigned base,
                                const unsigned* __restrict__ first, const unsigned long long* __restrict__ scan, unsigned long long* __restrict__ out) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const unsigned long long cell = i / (unsigned)t.t.n;
    const unsigned slot = (unsigned)(i % (unsigned)t.t.n);
    if (slot < (unsigned)t.s0) {
        out[i] = (unsigned long long)conn[cell * t.t.nv + slot];
        return;
    }
    const unsigned long long li = cell * (unsigned)t.S + (slot - (unsigned)t.s0);
    out[i] = (unsigned long long)base + (scan[first[li]] >> LABEL_SHIFT);
}

// Stage 5b: every winner writes its vertex and its transfer row; candidate 0, always a winner, closes the offsets.  Kept apart from
// k_refine_new_rows on purpose: the position repeats the host converters' operations in their order (no contraction), where the
// refinement sums in ascending global index:
//   1 parent    X[a]
//   2 parents   X[b] * 0.5 + X[a] * 0.5 (the sum commutes: the edge's direction does not matter), or (X[a] + X[b]) / 2 with kept vertices
//   4, 8        sum over the cell's local nodes a = 0 .. nv - 1 in order of X[a] * N_a, N_a = 1 / count on the face (cell), +0.0 off it
template <int MP, int D>
__global__ void k_elevate_rows(const double* __restrict__ verts, const int* __restrict__ conn, LabelTable t, unsigned nlab, unsigned base,
                               unsigned long long num_high, unsigned long long nnz, const unsigned* __restrict__ first,
                               const unsigned long long* __restrict__ scan, double* __restrict__ out_v, unsigned long long* __restrict__ off,
                               unsigned long long* __restrict__ idx, double* __restrict__ w) {
#pragma clang fp contract(off)
    const unsigned li = blockIdx.x * blockDim.x + threadIdx.x;
    if (li >= nlab || first[li] != li) return;
    if (li == 0) off[num_high] = nnz;
    const unsigned cell = li / (unsigned)t.S, slot = (unsigned)t.s0 + li % (unsigned)t.S;
    const int* ec = conn + (size_t)cell * t.t.nv;
    const signed char* par = t.t.par[slot];
    const int cnt = t.t.cnt[slot];
    const double wt = cnt == 1 ? 1.0 : cnt == 2 ? 0.5 : cnt == 4 ? 0.25 : 0.125;
    const unsigned long long s = scan[li];
    const size_t v = (size_t)base + (size_t)(s >> LABEL_SHIFT);
    const unsigned long long pos = (unsigned long long)base + (s & ((1ull << LABEL_SHIFT) - 1));
    off[v] = pos;
    if (cnt <= 2) {
        const size_t a = (size_t)ec[par[0]], b = (size_t)ec[par[cnt - 1]];
#pragma unroll
        for (int r = 0; r < D; ++r) {
            const double xa = verts[a * D + r], xb = verts[b * D + r];
            out_v[v * D + r] = cnt == 1 ? xa : t.keep ? (xa + xb) / 2.0 : xa * 0.5 + xb * 0.5;
        }
    } else {
        unsigned mask = 0u;
        for (int q = 0; q < cnt; ++q) mask |= 1u << par[q];
        double sum[D];
#pragma unroll
        for (int a = 0; a < MP; ++a) {
            if (a >= t.t.nv) break;
            const size_t g = (size_t)ec[a];
            const double Na = ((mask >> a) & 1u) ? wt : 0.0;
#pragma unroll
            for (int r = 0; r < D; ++r) {
                const double term = verts[g * D + r] * Na;
                sum[r] = a == 0 ? term : sum[r] + term;
            }
        }
#pragma unroll
        for (int r = 0; r < D; ++r) out_v[v * D + r] = sum[r];
    }
    unsigned k[MP];
    sorted_parent_tuple<MP>(ec, par, cnt, k);
#pragma unroll
    for (int q = 0; q < MP; ++q)
        if (q < cnt) {
            idx[pos + q] = k[q];
            w[pos + q] = wt;
        }
}

}  // namespace fenris_hip
