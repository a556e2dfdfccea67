#pragma once
// Degree coarsening kernels (engine_hierarchy.hip): the linear mesh on the vertex nodes of a quadratic mesh and
// the transfer from its vertices to all nodes.  Integer work only, apart from copying positions and writing the weights 1, 1/2, 1/4, 1/8.
// The only atomics are integer atomicMin / atomicOr, whose results do not depend on the order of arrival.
//
// An OCCURRENCE is one local node of one cell: id = cell * n + l.  A node's OWNER is its smallest occurrence; its ROLE says in which kind
// of slot it was seen (bit 0: a vertex slot, l < nv; bit 1: any other).  A non-vertex node's PARENTS are the nodes in the vertex slots
// of its edge, face or cell, as the sorted tuple of their fine indices: ascending fine index is ascending coarse index, because the
// coarse index is the rank among the vertex nodes.
#include <hip/hip_runtime.h>

#include "hierarchy_kernels.hpp"

namespace fenris_hip {

constexpr int COARSEN_SHIFT = 32;                // the scan's packing: vertex rank << 32 | row offset
// status words: the smallest offending node of each class
enum { COARSEN_ORPHAN = 0, COARSEN_MIXED = 1, COARSEN_MISMATCH = 2, COARSEN_STATUS_WORDS = 3 };

// the parent tuple of occurrence `id` as fine nodes
template <int MP>
__device__ __forceinline__ void coarsen_sorted_tuple(const int* __restrict__ conn, const CoarsenTable& t, unsigned id, unsigned (&k)[MP]) {
    const unsigned cell = id / (unsigned)t.n, l = id % (unsigned)t.n;
    sorted_parent_tuple<MP>(conn + (size_t)cell * t.n, t.par[l], t.cnt[l], k);
}

__global__ void k_coarsen_init(unsigned N, unsigned* __restrict__ owner, unsigned* __restrict__ role, unsigned* __restrict__ status) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < COARSEN_STATUS_WORDS) status[i] = COARSEN_NONE;
    if (i >= N) return;
    owner[i] = COARSEN_NONE;
    role[i] = 0u;
}

// Stage 1: owner and role of every node.  One thread per occurrence.
__global__ void k_coarsen_owner(const int* __restrict__ conn, CoarsenTable t, unsigned nocc, unsigned* __restrict__ owner,
                                unsigned* __restrict__ role) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nocc) return;
    const unsigned node = (unsigned)conn[i];
    atomicMin(&owner[node], i);
    atomicOr(&role[node], (i % (unsigned)t.n) < (unsigned)t.nv ? 1u : 2u);
}

// Stage 2: what the scan sums.  A vertex node: 1 << 32 (its rank among the vertex nodes is its coarse index) | 1 (its row holds itself);
// any other node: the number of its parents, from its owner occurrence.  A node of no cell and a node seen in both kinds of slot are
// refused: the smallest such node goes to the status words.
__global__ void k_coarsen_flags(CoarsenTable t, unsigned N, const unsigned* __restrict__ owner, const unsigned* __restrict__ role,
                                unsigned long long* __restrict__ val, unsigned* __restrict__ status) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const unsigned r = role[i];
    unsigned long long v = 0ull;
    if (r == 0u) atomicMin(&status[COARSEN_ORPHAN], i);
    else if (r == 3u) atomicMin(&status[COARSEN_MIXED], i);
    else if (r == 1u) v = (1ull << COARSEN_SHIFT) | 1ull;
    else v = (unsigned long long)t.cnt[owner[i] % (unsigned)t.n];
    val[i] = v;
}

// Stage 3: every occurrence in a non-vertex slot rebuilds its parent tuple and compares it with its node's owner's.
template <int MP>
__global__ void k_coarsen_check(const int* __restrict__ conn, CoarsenTable t, unsigned nocc, const unsigned* __restrict__ owner,
                                unsigned* __restrict__ status) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nocc || (i % (unsigned)t.n) < (unsigned)t.nv) return;
    const unsigned node = (unsigned)conn[i];
    const unsigned o = owner[node];
    if (o == i) return;
    unsigned mine[MP], other[MP];
    coarsen_sorted_tuple<MP>(conn, t, i, mine);
    coarsen_sorted_tuple<MP>(conn, t, o, other);
    bool eq = true;
#pragma unroll
    for (int a = 0; a < MP; ++a) eq = eq && mine[a] == other[a];
    if (!eq) atomicMin(&status[COARSEN_MISMATCH], node);
}

// Stage 5a: the transfer rows, one thread per fine node; a vertex node also records itself under its coarse index.  Thread N closes the
// offsets.  Consecutive threads write consecutive rows.
template <int MP>
__global__ void k_coarsen_rows(const int* __restrict__ conn, CoarsenTable t, unsigned N, unsigned long long nnz, const unsigned* __restrict__ owner,
                               const unsigned long long* __restrict__ scan, unsigned long long* __restrict__ off,
                               unsigned long long* __restrict__ idx, double* __restrict__ w, unsigned* __restrict__ vfine) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == N) off[N] = nnz;
    if (i >= N) return;
    const unsigned long long s = scan[i];
    const unsigned long long pos = s & ((1ull << COARSEN_SHIFT) - 1);
    const unsigned o = owner[i];
    const int cnt = t.cnt[o % (unsigned)t.n];
    off[i] = pos;
    if (cnt == 1) {
        const unsigned j = (unsigned)(s >> COARSEN_SHIFT);
        idx[pos] = j;
        w[pos] = 1.0;
        vfine[j] = i;
        return;
    }
    unsigned k[MP];
    coarsen_sorted_tuple<MP>(conn, t, o, k);
    const double wt = cnt == 2 ? 0.5 : cnt == 4 ? 0.25 : 0.125;
#pragma unroll
    for (int q = 0; q < MP; ++q)
        if (q < cnt) {
            idx[pos + q] = scan[k[q]] >> COARSEN_SHIFT;
            w[pos + q] = wt;
        }
}

// Stage 5b: the coarse cells.  One thread per node of a coarse cell: consecutive threads write consecutive words.
__global__ void k_coarsen_cells(const int* __restrict__ conn, CoarsenTable t, unsigned long long total, const unsigned long long* __restrict__ scan,
                                unsigned long long* __restrict__ out) {
    const unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const unsigned long long cell = i / (unsigned)t.nv;
    const unsigned a = (unsigned)(i % (unsigned)t.nv);
    out[i] = scan[conn[cell * t.n + a]] >> COARSEN_SHIFT;
}

// Stage 5c: the coarse vertices, one thread each: the fine position, bit for bit, and the fine index.
template <int D>
__global__ void k_coarsen_vertices(const double* __restrict__ verts, unsigned M, const unsigned* __restrict__ vfine, double* __restrict__ out_v,
                                   unsigned long long* __restrict__ vertex_nodes) {
    const unsigned j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= M) return;
    const unsigned i = vfine[j];
#pragma unroll
    for (int r = 0; r < D; ++r) out_v[(size_t)j * D + r] = verts[(size_t)i * D + r];
    vertex_nodes[j] = i;
}

}  // namespace fenris_hip
