#pragma once
// Degree elevation kernels (engine_elevate.hip): the quadratic mesh over a linear one and the transfer from the
// linear vertices to all of its nodes, numbered as the sequential sweeps fh_refine_to_quadratic and fh_hex8_to_hex27 number them
// (host_inputs.cpp).  Integer work only up to the row kernel: no atomics.
//
// A CANDIDATE is one labelled slot of one cell: li = cell * S + j names local node s0 + j of the high cell.  Tet10, Hex20 and Hex27 label
// every slot (s0 = 0: the old vertex indices are not kept); Tri6 and Quad9 keep the old vertices and label the other slots (s0 = nv).
// Ascending li is the order of the sweep.  Two candidates are the same node iff their sorted tuples of parent linear vertices are equal;
// the node takes the rank of its FIRST candidate (the smallest li) among the first candidates, and that candidate alone -- the WINNER --
// computes its position, from its own cell in its local node order, and writes its transfer row.  A cell centre is the last slot of its
// cell, belongs to no other cell and is its own winner without matching: the first Sm <= S slots of a cell go through the sort.
#include <hip/hip_runtime.h>

#include "hierarchy_kernels.hpp"   // CoarsenTable: the parents of every local node of the high kind; sorted_parent_tuple; k_refine_coarse_rows

namespace fenris_hip {

struct ElevateTable {
    CoarsenTable t;   // of the high kind; the cells read are the linear ones, t.nv nodes each
    int s0, S, Sm;    // first labelled slot; labelled slots per cell (n - s0); ... of which matched through the sort
    int keep;         // Tri6, Quad9: old vertices keep their indices, and an edge midpoint is (X[a] + X[b]) / 2, not 0.5 X[a] + 0.5 X[b]
};

constexpr int ELEVATE_SHIFT = 33;   // the scan's packing: rank << 33 | row offset (at most 64 parents in 27 slots: below 2^33)

template <int MP>
__device__ __forceinline__ void elevate_sorted_tuple(const int* __restrict__ conn, const ElevateTable& t, unsigned li, unsigned (&k)[MP]) {
    const unsigned cell = li / (unsigned)t.S, slot = (unsigned)t.s0 + li % (unsigned)t.S;
    sorted_parent_tuple<MP>(conn + (size_t)cell * t.t.nv, t.t.par[slot], t.t.cnt[slot], k);
}

// Stage 1: the sort key of every matched candidate: its two smallest parents, `bits` bits each, the smallest in the high half; a vertex
// has one parent and takes `pad` = num_vertices < 2^bits for the other, so it shares its bucket with no edge.  With at most two parents
// per candidate (MP == 2) the key is the whole tuple.  Consecutive threads write consecutive keys and ids.
template <int MP>
__global__ void k_elevate_keys(const int* __restrict__ conn, ElevateTable t, unsigned nsort, unsigned pad, int bits,
                               unsigned long long* __restrict__ keys, unsigned* __restrict__ ids) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nsort) return;
    const unsigned li = (i / (unsigned)t.Sm) * (unsigned)t.S + i % (unsigned)t.Sm;
    unsigned k[MP];
    elevate_sorted_tuple<MP>(conn, t, li, k);
    const unsigned k1 = k[1] == COARSEN_NONE ? pad : k[1];
    keys[i] = ((unsigned long long)k[0] << bits) | (unsigned long long)k1;
    ids[i] = li;
}

// Stage 3 (after the stable sort by key: every bucket holds its candidates ascending): first[li] = the smallest candidate with the same
// full tuple, found by walking the bucket towards its head; with MP == 2 the head is the answer.  val[li] packs what the scan sums and
// is zero unless the candidate is a winner: 1 << 33 (its rank) | its number of parents (the offset of its transfer row).  Thread `cell`
// also enters the centre of that cell, where the kind has one.
template <int MP>
__global__ void k_elevate_first(const int* __restrict__ conn, ElevateTable t, unsigned nsort, unsigned E, const unsigned long long* __restrict__ keys,
                                const unsigned* __restrict__ ids, unsigned* __restrict__ first, unsigned long long* __restrict__ val) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nsort) return;
    if (t.S != t.Sm && i < E) {
        const unsigned centre = i * (unsigned)t.S + (unsigned)t.Sm;
        first[centre] = centre;
        val[centre] = (1ull << ELEVATE_SHIFT) | (unsigned long long)t.t.cnt[t.t.n - 1];
    }
    const unsigned long long key = keys[i];
    const unsigned li = ids[i];
    unsigned f = li;
    unsigned mine[MP], other[MP];
    if (MP > 2) elevate_sorted_tuple<MP>(conn, t, li, mine);
    for (long long j = (long long)i - 1; j >= 0 && keys[j] == key; --j) {
        const unsigned oj = ids[j];
        if (MP == 2) { f = oj; continue; }
        elevate_sorted_tuple<MP>(conn, t, oj, other);
        bool eq = true;
#pragma unroll
        for (int a = 0; a < MP; ++a) eq = eq && mine[a] == other[a];
        if (eq) f = oj;
    }
    first[li] = f;
    val[li] = f == li ? ((1ull << ELEVATE_SHIFT) | (unsigned long long)t.t.cnt[(unsigned)t.s0 + li % (unsigned)t.S]) : 0ull;
}

// Stage 5a: the high cells.  One thread per node of a cell: consecutive threads write consecutive words.  A labelled slot reads the rank
// of its winner; `base` is the number of kept vertices (0 where none is kept).
__global__ void k_elevate_cells(const int* __restrict__ conn, ElevateTable t, unsigned long long total, unsigned base,
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
    out[i] = (unsigned long long)base + (scan[first[li]] >> ELEVATE_SHIFT);
}

// Stage 5b: every winner writes its vertex and its transfer row; candidate 0, always a winner, closes the offsets.  The position repeats
// the host's operations in the host's order (no contraction):
//   1 parent    X[a]
//   2 parents   X[b] * 0.5 + X[a] * 0.5 (the sum commutes: the edge's direction does not matter), or (X[a] + X[b]) / 2 with kept vertices
//   4, 8        sum over the cell's local nodes a = 0 .. nv - 1 in order of X[a] * N_a, N_a = 1 / count on the face (cell), +0.0 off it
template <int MP, int D>
__global__ void k_elevate_rows(const double* __restrict__ verts, const int* __restrict__ conn, ElevateTable t, unsigned nlab, unsigned base,
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
    const size_t v = (size_t)base + (size_t)(s >> ELEVATE_SHIFT);
    const unsigned long long pos = (unsigned long long)base + (s & ((1ull << ELEVATE_SHIFT) - 1));
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
