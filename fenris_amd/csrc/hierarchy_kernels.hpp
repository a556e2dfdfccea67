#pragma once
// What the mesh hierarchy passes share (refine_kernels.hpp, coarsen_kernels.hpp, elevate_kernels.hpp; engine_hierarchy.hip, DESIGN.md
// section 3.6.3): the parent table of a quadratic kind, the sorted parent tuple of a node, the labelling of new nodes by their parents
// (refinement and elevation), and the rows of vertices that keep their indices.  Integer work only: no atomics.
//
// LABELLING.  A CANDIDATE is one labelled slot of one cell: li = cell * S + j names local node s0 + j of the table.  Ascending li is the
// order of a sequential sweep over the cells.  Two candidates are the same node iff their sorted tuples of parent vertices are equal; the
// node takes the rank of its FIRST candidate (the smallest li) among the first candidates -- the label the host sweeps hand out
// (host_inputs.cpp) -- and that candidate alone, the WINNER, writes the node's position and transfer row.  The first Sm <= S slots of a
// cell are matched through a sort; the others (a cell centre that is the last slot of its cell and belongs to no other) are their own
// winners without it.
#include <hip/hip_runtime.h>

namespace fenris_hip {

constexpr int COARSEN_MAX_NODES = 27;

// The parents of every local node of a cell kind, by value in the kernel arguments.
struct CoarsenTable {
    int n, nv;                                   // nodes per cell; vertex slots per cell (the first nv local nodes)
    signed char cnt[COARSEN_MAX_NODES];          // parents of local node l: 1 (a vertex slot: itself), 2, 4 or 8
    signed char par[COARSEN_MAX_NODES][8];       // ... as local nodes < nv
};

// the table of a quadratic kind and its linear kind; false for a kind without one (engine_hierarchy.hip)
bool coarsen_table(int kind, CoarsenTable& t, int& linear_kind);

// The candidates of a labelling.  The cells read are the linear ones, t.nv nodes each.
struct LabelTable {
    CoarsenTable t;   // the parents of every local node: the high kind of an elevation, the old and the new points of a refinement
    int s0, S, Sm;    // first labelled slot; labelled slots per cell (n - s0); ... of which matched through the sort
    int keep;         // the old vertices keep their indices (s0 = nv) and the new nodes are numbered after them; an elevation then places an
                      // edge midpoint at (X[a] + X[b]) / 2, not 0.5 X[a] + 0.5 X[b]
};

constexpr unsigned COARSEN_NONE = 0xFFFFFFFFu;   // padding of a tuple, and "no node" in the status words
constexpr int LABEL_SHIFT = 33;   // the scan's packing: rank << 33 | row offset (at most 64 parents in 27 slots, < 2^31 candidates: below 2^33)

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

// the parent tuple of candidate li
template <int MP>
__device__ __forceinline__ void label_sorted_tuple(const int* __restrict__ conn, const LabelTable& t, unsigned li, unsigned (&k)[MP]) {
    const unsigned cell = li / (unsigned)t.S, slot = (unsigned)t.s0 + li % (unsigned)t.S;
    sorted_parent_tuple<MP>(conn + (size_t)cell * t.t.nv, t.t.par[slot], t.t.cnt[slot], k);
}

// Stage 1: the sort key of every matched candidate: its two smallest parents, `bits` bits each, the smallest in the high half (as
// k_face_keys); a vertex has one parent and takes `pad` = num_vertices < 2^bits for the other, so it shares its bucket with no edge.
// With at most two parents per candidate (MP == 2) the key is the whole tuple.  Consecutive threads write consecutive keys and ids.
template <int MP>
__global__ void k_label_keys(const int* __restrict__ conn, LabelTable t, unsigned nsort, unsigned pad, int bits,
                             unsigned long long* __restrict__ keys, unsigned* __restrict__ ids) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nsort) return;
    const unsigned li = (i / (unsigned)t.Sm) * (unsigned)t.S + i % (unsigned)t.Sm;
    unsigned k[MP];
    label_sorted_tuple<MP>(conn, t, li, k);
    const unsigned k1 = k[1] == COARSEN_NONE ? pad : k[1];
    keys[i] = ((unsigned long long)k[0] << bits) | (unsigned long long)k1;
    ids[i] = li;
}

// Stage 3 (after the stable sort by key: every bucket holds its candidates ascending): first[li] = the smallest candidate with the same
// full tuple, found by walking the bucket towards its head; with MP == 2 the head is the answer.  val[li] packs what the scan sums and
// is zero unless the candidate is a winner: 1 << 33 (its rank) | its number of parents (the offset of its transfer row).  Thread `cell`
// also enters the unmatched centre of that cell, where the table has one.
template <int MP>
__global__ void k_label_first(const int* __restrict__ conn, LabelTable t, unsigned nsort, unsigned E, const unsigned long long* __restrict__ keys,
                              const unsigned* __restrict__ ids, unsigned* __restrict__ first, unsigned long long* __restrict__ val) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nsort) return;
    if (t.S != t.Sm && i < E) {
        const unsigned centre = i * (unsigned)t.S + (unsigned)t.Sm;
        first[centre] = centre;
        val[centre] = (1ull << LABEL_SHIFT) | (unsigned long long)t.t.cnt[t.t.n - 1];
    }
    const unsigned long long key = keys[i];
    const unsigned li = ids[i];
    unsigned f = li;
    unsigned mine[MP], other[MP];
    if (MP > 2) label_sorted_tuple<MP>(conn, t, li, mine);
    for (long long j = (long long)i - 1; j >= 0 && keys[j] == key; --j) {
        const unsigned oj = ids[j];
        if (MP == 2) { f = oj; continue; }
        label_sorted_tuple<MP>(conn, t, oj, other);
        bool eq = true;
#pragma unroll
        for (int a = 0; a < MP; ++a) eq = eq && mine[a] == other[a];
        if (eq) f = oj;
    }
    first[li] = f;
    val[li] = f == li ? ((1ull << LABEL_SHIFT) | (unsigned long long)t.t.cnt[(unsigned)t.s0 + li % (unsigned)t.S]) : 0ull;
}

// The vertices that keep their indices (the coarse ones of a refinement; the old ones under Tri6 and Quad9): positions copied, transfer
// rows the identity.  Thread N closes the offsets.
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
