#pragma once
// Uniform refinement kernels (engine_refine.hip).  Integer work only up to the vertex kernel: no atomics.
//
// An OCCURRENCE is one new point of one cell: id = cell * P + p, p the place of the point in the kind's list.  Two occurrences are the
// same fine vertex iff their sorted tuples of parent coarse vertices are equal; the fine vertex takes the place of its FIRST occurrence
// (the smallest id) among the new vertices -- the label a sequential sweep over the cells hands out (refine_hex8_uniform,
// host_inputs.cpp).
//
// Tri3: the children [0,3,5] [3,1,4] [5,4,2] [3,4,5] are the reference's [a,d,f] [d,b,e] [f,e,c] [d,e,f] (src/mesh/refinement/detail.rs:
// 116-127).  Only the vertex LABELS differ from the reference's: it labels the old vertices by first appearance too, here they keep
// their indices.
#include <hip/hip_runtime.h>

#include "hierarchy_kernels.hpp"

namespace fenris_hip {

constexpr int REFINE_MAX_POINTS = 19;   // Hex8: the 3x3x3 lattice without its 8 corners

// The new points and the children of a cell kind, by value in the kernel arguments.  Local index n + p names new point p.
struct RefineTable {
    int n, P, C;                                 // nodes per cell, new points per cell, children per cell
    signed char cnt[REFINE_MAX_POINTS];          // parents of point p: 2, 4 or 8
    signed char par[REFINE_MAX_POINTS][8];       // ... as local nodes
    signed char child[8][8];                     // child k, node a: local index
};

constexpr unsigned REFINE_NONE = 0xFFFFFFFFu;    // padding of a tuple: sorts last, so the number of parents is part of the tuple

// the parent tuple of occurrence `id`, ascending, padded with REFINE_NONE.  Odd-even transposition with compile-time indices: the tuple
// stays in registers.
template <int MP>
__device__ __forceinline__ void refine_sorted_tuple(const int* __restrict__ conn, const RefineTable& t, unsigned id, unsigned (&k)[MP]) {
    const unsigned cell = id / (unsigned)t.P, p = id % (unsigned)t.P;
    const int* ec = conn + (size_t)cell * t.n;
    const int cnt = t.cnt[p];
#pragma unroll
    for (int a = 0; a < MP; ++a) k[a] = a < cnt ? (unsigned)ec[t.par[p][a]] : REFINE_NONE;
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

template <int MP>
__device__ __forceinline__ bool refine_tuple_equal(const unsigned (&a)[MP], const unsigned (&b)[MP]) {
    bool eq = true;
#pragma unroll
    for (int i = 0; i < MP; ++i) eq = eq && a[i] == b[i];
    return eq;
}

// Stage 1: the sort key of every occurrence: its two smallest parents, `bits` bits each, the smallest in the high half (as k_face_keys).
// Cell-centre points are unique by construction and take part all the same: their ids hold their places in the order of appearance.
template <int MP>
__global__ void k_refine_keys(const int* __restrict__ conn, RefineTable t, unsigned nocc, int bits, unsigned long long* __restrict__ keys,
                              unsigned* __restrict__ ids) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nocc) return;
    unsigned k[MP];
    refine_sorted_tuple<MP>(conn, t, i, k);
    keys[i] = ((unsigned long long)k[0] << bits) | (unsigned long long)k[1];
    ids[i] = i;
}

// Stage 3 (after the stable sort by key: every bucket holds its ids ascending): first[id] = the smallest id with the same full tuple,
// found by walking the bucket towards its head.  With two parents per point the key is the whole tuple and the head is the answer.
// val[id] packs what the scan of stage 4 sums, and is zero unless the occurrence is a first one: 1 << 33 (the rank among the new
// vertices) | its number of parents (the offset of its transfer row).  The low part stays below 2^33: the parents of one cell's points
// number at most 56 of 19 (Hex8), and nocc < 2^31.
template <int MP>
__global__ void k_refine_first(const int* __restrict__ conn, RefineTable t, unsigned nocc, const unsigned long long* __restrict__ keys,
                               const unsigned* __restrict__ ids, unsigned* __restrict__ first, unsigned long long* __restrict__ val) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nocc) return;
    const unsigned long long key = keys[i];
    const unsigned id = ids[i];
    unsigned f = id;
    unsigned mine[MP], other[MP];
    if (MP > 2) refine_sorted_tuple<MP>(conn, t, id, mine);
    for (long long j = (long long)i - 1; j >= 0 && keys[j] == key; --j) {
        const unsigned oj = ids[j];
        if (MP == 2) { f = oj; continue; }
        refine_sorted_tuple<MP>(conn, t, oj, other);
        if (refine_tuple_equal<MP>(mine, other)) f = oj;
    }
    first[id] = f;
    val[id] = f == id ? ((1ull << 33) | (unsigned long long)t.cnt[id % (unsigned)t.P]) : 0ull;
}

// Stage 5a: the fine index of every occurrence: N + the rank of its tuple's first occurrence
__global__ void k_refine_fine_index(unsigned nocc, unsigned N, const unsigned* __restrict__ first, const unsigned long long* __restrict__ scan,
                                    unsigned* __restrict__ fine) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nocc) return;
    fine[i] = N + (unsigned)(scan[first[i]] >> 33);
}

// Stage 5b: the children.  One thread per node of a child: consecutive threads write consecutive words.
__global__ void k_refine_children(const int* __restrict__ conn, RefineTable t, unsigned long long total, const unsigned* __restrict__ fine,
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

// Stage 5c, new part: every first occurrence writes its vertex and its transfer row.  The position is the sum of the parents in
// ascending index times 1 / count -- the operations and their order of refine_hex8_uniform (host_inputs.cpp), so the bits are the
// host's: the sum starts at 0.0, the product is a product alone (nothing to contract it with), and 1 / count is exact.
template <int MP, int D>
__global__ void k_refine_new_rows(const double* __restrict__ verts, const int* __restrict__ conn, RefineTable t, unsigned nocc, unsigned N,
                                  const unsigned* __restrict__ first, const unsigned long long* __restrict__ scan, double* __restrict__ out_v,
                                  unsigned long long* __restrict__ off, unsigned long long* __restrict__ idx, double* __restrict__ w) {
#pragma clang fp contract(off)
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nocc || first[i] != i) return;
    unsigned k[MP];
    refine_sorted_tuple<MP>(conn, t, i, k);
    const int cnt = t.cnt[i % (unsigned)t.P];
    const double wt = cnt == 2 ? 0.5 : cnt == 4 ? 0.25 : 0.125;
    const unsigned long long s = scan[i];
    const size_t v = (size_t)N + (size_t)(s >> 33);
    const unsigned long long pos = (unsigned long long)N + (s & ((1ull << 33) - 1));
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
