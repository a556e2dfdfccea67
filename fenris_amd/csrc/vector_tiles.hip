// Residual vector through element TILES (round 4): the element vectors never reach HBM.
//
// Round 3's two passes (element_pass.hpp) wrote every element vector to scratch (Hex8 elasticity: 192 bytes per element) and read it back
// per node: 1.9 GB each way on Hex8 216^3 for 1.06 GB of algorithmic traffic.  Here the elements are cut into TILES of 256 that are
// compact in space (consecutive runs of the Morton order of the element centroids: 8 x 8 x 4 bricks on a structured mesh, clusters on
// any other), one workgroup per tile:
//
//  * every thread computes its element's vector in registers exactly as before (element_pass_body: assemble_element_elliptic_vector,
//    src/assembly/local/elliptic.rs:457-531) and leaves it in LDS, stage[a][c][thread];
//  * the tile's DISTINCT nodes (~405 of a brick's 2048 (element, local node) entries) are summed from LDS, one thread per node over its
//    entries in ascending (element, local node) order, and only these partial sums go to HBM: partial[P][S], ~1.6 per element
//    instead of 8 (38 instead of 192 bytes per Hex8 element);
//  * the node pass (k_vector_from_partials) adds the partials of every node in ascending tile order (1.6 on average) to the output:
//    the work of VectorAssembler::assemble_vector_into's add_local_to_global (global.rs:582-608, 770-796) without atomics, in an order
//    fixed by the tables: bitwise reproducible.
//
// The tables (tile membership, local node numbers, in-tile adjacency, node -> partials) depend on the connectivity only (the vertex
// coordinates merely decide how compact the tiles are) and are built on the device: Morton keys, hipcub radix sort, one workgroup
// per tile that sorts its 2048 (node, entry) keys in LDS, two scans.  Element masks (fh_set_active_elements: the multi-GPU partitions)
// zero the inactive elements' contributions.
//
// Every route over the tiles repeats bit for bit and agrees with the others because there is ONE copy of the load pattern and of the
// order of the additions: TilePass is the frame of every element pass (the tile, the element, the gathers, the staging store, the
// tile's node sums) and node_partials_sum the ordered sum of every node pass (block_partial_store: the per-workgroup partial some of
// them leave).  A new tile kernel is a body between TilePass's begin, its gathers and finish; a new node pass is a per-node statement
// after node_partials_sum.  Neither reads the tables itself.
#include <hipcub/hipcub.hpp>

#include <vector>

#include "dispatch.hpp"
#include "element_pass.hpp"
#include "vector_tiles.hpp"

namespace fenris_hip {

namespace {

constexpr int VT_TS = 256;   // elements per tile = threads per workgroup of the element pass (the kernels take it as a template parameter)

struct Box3 { double lo[3], scale[3]; };

__global__ void __launch_bounds__(256) k_vt_bbox(const double* verts, int num_nodes, int D, double* out /* [grid][6] */) {
    __shared__ double red[6][256];
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (int v = blockIdx.x * 256 + threadIdx.x; v < num_nodes; v += gridDim.x * 256)
        for (int i = 0; i < D; ++i) {
            const double x = verts[(size_t)v * D + i];
            if (x < lo[i]) lo[i] = x;     // (NaN coordinates compare false: ignored)
            if (x > hi[i]) hi[i] = x;
        }
    for (int i = 0; i < 3; ++i) { red[i][threadIdx.x] = lo[i]; red[3 + i][threadIdx.x] = hi[i]; }
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int i = 0; i < 3; ++i) {
                red[i][threadIdx.x] = fmin(red[i][threadIdx.x], red[i][threadIdx.x + s]);
                red[3 + i][threadIdx.x] = fmax(red[3 + i][threadIdx.x], red[3 + i][threadIdx.x + s]);
            }
        __syncthreads();
    }
    if (threadIdx.x < 6) out[(size_t)blockIdx.x * 6 + threadIdx.x] = red[threadIdx.x][0];
}

__device__ __forceinline__ unsigned long long vt_spread21(unsigned long long v) {   // 21 bits -> every third bit
    v &= 0x1fffffull;
    v = (v | (v << 32)) & 0x1f00000000ffffull;
    v = (v | (v << 16)) & 0x1f0000ff0000ffull;
    v = (v | (v << 8)) & 0x100f00f00f00f00full;
    v = (v | (v << 4)) & 0x10c30c30c30c30c3ull;
    v = (v | (v << 2)) & 0x1249249249249249ull;
    return v;
}

__global__ void __launch_bounds__(256) k_vt_morton(const int* conn, int n, long long E, const double* verts, int D, int num_nodes, Box3 box,
                                                   unsigned long long* keys, int* vals, int* bad) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    double c[3] = {0.0, 0.0, 0.0};
    for (int a = 0; a < n; ++a) {
        const int v = conn[(size_t)e * n + a];
        if (v < 0 || v >= num_nodes) { *bad = 1; continue; }
        for (int i = 0; i < D; ++i) c[i] += verts[(size_t)v * D + i];
    }
    unsigned long long key = 0;
    for (int i = 0; i < D; ++i) {
        double q = (c[i] / n - box.lo[i]) * box.scale[i];
        if (!(q >= 0.0)) q = 0.0;          // also NaN
        if (q > 2097151.0) q = 2097151.0;
        key |= vt_spread21((unsigned long long)q) << i;
    }
    keys[e] = key;
    vals[e] = (int)e;
}

template <typename T>
__device__ __forceinline__ void vt_bitonic_sort(T* d, int M, int nthreads) {   // ascending, M a power of two
    for (int k = 2; k <= M; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < M; i += nthreads) {
                const int o = i ^ j;
                if (o > i) {
                    const T x = d[i], y = d[o];
                    if ((x > y) == ((i & k) == 0)) { d[i] = y; d[o] = x; }
                }
            }
            __syncthreads();
        }
}

constexpr unsigned long long VT_PAD = ~0ull;

// one workgroup per tile.  FILL = false: number of distinct nodes of the tile;  FILL = true: all tables of the tile
template <bool FILL, int TS>
__global__ void __launch_bounds__(TS) k_vt_tile_tables(const int* order, long long E, const int* conn, int n, unsigned* tile_cnt, const unsigned* noff,
                                                        int* elem, int* tconn, unsigned short* la_off, unsigned short* la, unsigned* p_node) {   // p_node: global node of every partial
    __shared__ unsigned long long key[TS * 8];
    __shared__ unsigned scan[TS];
    const int tile = blockIdx.x, t = threadIdx.x;
    const long long idx = (long long)tile * TS + t;
    key[t] = idx < E ? (unsigned long long)(unsigned)order[idx] : VT_PAD;
    __syncthreads();
    vt_bitonic_sort(key, TS, TS);                                  // elements ascending inside the tile
    const long long el = key[t] == VT_PAD ? -1 : (long long)key[t];
    __syncthreads();
    if (FILL) elem[idx] = (int)el;
    const int M = TS * n;                                       // <= 2048 entries thread n + a
    // (threads without an element read the tile's first element: the kernel computes on every lane and drops their results)
    const long long er = el >= 0 ? el : (long long)key[0];
    for (int a = 0; a < n; ++a) {
        const int node = conn[(size_t)er * n + a];
        if (FILL) tconn[((size_t)tile * n + a) * TS + t] = node;
    }
    __syncthreads();
    for (int i = t; i < TS * 8; i += TS) key[i] = VT_PAD;
    __syncthreads();
    if (el >= 0)
        for (int a = 0; a < n; ++a) key[t * n + a] = ((unsigned long long)(unsigned)conn[(size_t)el * n + a] << 11) | (unsigned)(t * n + a);
    __syncthreads();
    vt_bitonic_sort(key, TS * 8, TS);                                 // by node, then by entry; the padding last
    // heads of the runs of equal nodes: eight consecutive places per thread, then a scan over the threads
    unsigned heads = 0, nvalid = 0;
    for (int j = 0; j < 8; ++j) {
        const int i = t * 8 + j;
        const unsigned long long k = key[i];
        if (k != VT_PAD) {
            ++nvalid;
            if (i == 0 || (key[i - 1] >> 11) != (k >> 11)) ++heads;
        }
    }
    scan[t] = heads;
    __syncthreads();
    for (int s = 1; s < TS; s <<= 1) {
        const unsigned v = t >= s ? scan[t - s] : 0u;
        __syncthreads();
        scan[t] += v;
        __syncthreads();
    }
    const unsigned U = scan[TS - 1];
    if (!FILL) {
        if (t == 0) tile_cnt[tile] = U;
        return;
    }
    // number of valid entries = M minus the padding of absent elements: count through a second use of the scan array
    unsigned ln = scan[t] - heads;                               // distinct nodes before this thread's places
    __syncthreads();
    scan[t] = nvalid;
    __syncthreads();
    for (int s = TS / 2; s > 0; s >>= 1) {
        if (t < s) scan[t] += scan[t + s];
        __syncthreads();
    }
    const unsigned total = scan[0];
    const unsigned base = noff[tile];
    unsigned short* lo = la_off + base + tile;
    unsigned short* lat = la + (size_t)tile * M;
    for (int j = 0; j < 8; ++j) {
        const int i = t * 8 + j;
        const unsigned long long k = key[i];
        if (k == VT_PAD) continue;
        const bool head = i == 0 || (key[i - 1] >> 11) != (k >> 11);
        if (head) {
            lo[ln] = (unsigned short)i;
            p_node[base + ln] = (unsigned)(k >> 11);
            ++ln;
        }
        const unsigned ent = (unsigned)(k & 2047u);
        lat[i] = (unsigned short)ent;
    }
    if (t == 0) lo[U] = (unsigned short)total;
}

__global__ void __launch_bounds__(256) k_vt_count(const unsigned* p_node, unsigned P, unsigned* deg) {
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p < P) atomicAdd(&deg[p_node[p]], 1u);
}
__global__ void __launch_bounds__(256) k_vt_fill(const unsigned* p_node, unsigned P, const unsigned* np_off, unsigned* cursor, unsigned* np_idx) {
    const unsigned p = blockIdx.x * 256u + threadIdx.x;
    if (p < P) {
        const unsigned v = p_node[p];
        np_idx[np_off[v] + atomicAdd(&cursor[v], 1u)] = p;
    }
}
__global__ void __launch_bounds__(256) k_vt_sort_lists(const unsigned* np_off, unsigned* np_idx, int num_nodes) {   // short lists: insertion sort
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= num_nodes) return;
    const unsigned k0 = np_off[v], k1 = np_off[v + 1];
    for (unsigned i = k0 + 1; i < k1; ++i) {
        const unsigned x = np_idx[i];
        unsigned j = i;
        while (j > k0 && np_idx[j - 1] > x) { np_idx[j] = np_idx[j - 1]; --j; }
        np_idx[j] = x;
    }
}

// ---- the element pass over tiles
// tile of workgroup b when the grid is 8 ceil(T / 8) workgroups: XCD b mod 8 walks the tiles [x c, (x + 1) c), c = ceil(T / 8)
__device__ __forceinline__ int xcd_tile(int b, int ntiles) {
    const int c = (ntiles + 7) >> 3;
    return (b & 7) * c + (b >> 3);
}
// what a tile's workgroup needs for the node sums, requested before the arithmetic and landing behind it: the tile's entries (256 N
// sixteen-bit values: N / 4 eight-byte pieces per thread) and the starts of the first 512 distinct nodes
template <int N, int TS>
struct TileSums {
    static constexpr int EW = (N * 2 + 7) / 8;
    unsigned base, U;
    const unsigned short* lo;
    uint2 ent_w[EW];
    unsigned short st0[2], st1[2];
    __device__ __forceinline__ void request(const VecTiles& t, int tile, int tid) {
        base = t.noff[tile];
        U = t.noff[tile + 1] - base;
        lo = t.la_off + base + tile;
        const uint2* la8 = reinterpret_cast<const uint2*>(t.la + (size_t)tile * (TS * N));   // (TS N x 2 bytes per tile: 8-byte aligned for even N)
        if constexpr (N % 4 == 0) {
#pragma unroll
            for (int w = 0; w < EW; ++w) ent_w[w] = la8[w * TS + tid];
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const unsigned p = tid + TS * j;
            st0[j] = st1[j] = 0;
            if (p < U) { st0[j] = lo[p]; st1[j] = lo[p + 1]; }
        }
    }
    // stage[a][c][thread] holds the element vectors (SV components); ents: LDS place for the entries.  Ends with the partials stored.
    template <int SV>
    __device__ __forceinline__ void sum(const VecTiles& t, int tile, int tid, const double* stage, unsigned short* ents, double* partial) {
        if constexpr (N % 4 == 0) {
            uint2* e8 = reinterpret_cast<uint2*>(ents);
#pragma unroll
            for (int w = 0; w < EW; ++w) e8[w * TS + tid] = ent_w[w];
        }
        __syncthreads();
        const unsigned short* la = t.la + (size_t)tile * (TS * N);
        auto sum_node = [&](unsigned p, unsigned k0, unsigned k1) {
            double acc[SV];
#pragma unroll
            for (int c = 0; c < SV; ++c) acc[c] = 0.0;
            for (unsigned k = k0; k < k1; ++k) {
                const unsigned ent = (N % 4 == 0) ? ents[k] : la[k], tt = ent / (unsigned)N, aa = ent - tt * (unsigned)N;
#pragma unroll
                for (int c = 0; c < SV; ++c) acc[c] += stage[(aa * SV + c) * TS + tt];
            }
#pragma unroll
            for (int c = 0; c < SV; ++c) partial[(size_t)(base + p) * SV + c] = acc[c];
        };
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const unsigned p = tid + TS * j;
            if (p < U) sum_node(p, st0[j], st1[j]);
        }
        for (unsigned p = tid + 2 * TS; p < U; p += TS) sum_node(p, lo[p], lo[p + 1]);   // (tiles of scattered elements)
    }
};

// The frame of every element pass over tiles.  A kernel declares the LDS (stage[N SV TS], ents[(N % 4 == 0) ? TS N : 4]) and is
// begin, one walk over the nodes with the gathers it needs, its own body, finish; what differs between kernels stands between these
// calls.  SUMS = false: a pass without node sums (the energy), which shares begin and the gathers only.
template <int N, int TS, bool SUMS = true>
struct TilePass {
    int tile, tid, el, ec;   // ec: el, or 0 for a thread without an element (it computes like the others and its result is dropped)
    bool live;               // the thread has an element and the mask (may be null) keeps it
    int nd[N];
    TileSums<N, TS> ts;
    // false: the workgroup has no tile.  Workgroup b runs on XCD b mod 8 (round-robin dispatch): every XCD takes one contiguous eighth of
    // the tiles, so that tiles that are neighbours in space (consecutive in the Morton order) share their boundary nodes' coordinates and u
    // through one L2.  The tables of the node sums are requested here, before the gathers and the arithmetic, and land behind them.  The
    // tile's connectivity comes from a table laid out by tile thread (tconn[tile][a][thread]: coalesced, and not behind the load of the
    // element id), all N nodes before the first gather.
    __device__ __forceinline__ bool begin(const VecTiles& t, const unsigned char* active) {
        tile = xcd_tile((int)blockIdx.x, t.ntiles), tid = threadIdx.x;
        if (tile >= t.ntiles) return false;
        el = t.elem[(size_t)tile * TS + tid];
        live = el >= 0 && (!active || active[el] != 0);
        ec = el >= 0 ? el : 0;
        if constexpr (SUMS) ts.request(t, tile, tid);
#pragma unroll
        for (int n = 0; n < N; ++n) nd[n] = t.tconn[((size_t)tile * N + n) * TS + tid];
        return true;
    }
    // the gathers of local node n (the kernel walks the nodes, what it needs of a node side by side): the vertex coordinates; a nodal
    // field (a null pointer reads as zero); a field whose entries at the nodes of dmask (may be null) read as zero
    template <int D>
    __device__ __forceinline__ void coords(int n, const double* verts, double (&x)[D]) const {
#pragma unroll
        for (int i = 0; i < D; ++i) x[i] = verts[(size_t)nd[n] * D + i];
    }
    template <int S>
    __device__ __forceinline__ void field(int n, const double* u, double (&v)[S]) const {
#pragma unroll
        for (int k = 0; k < S; ++k) v[k] = u ? u[(size_t)nd[n] * S + k] : 0.0;
    }
    template <int S>
    __device__ __forceinline__ void field_masked(int n, const double* x, const unsigned char* dmask, double (&v)[S]) const {
        const unsigned fixed = node_dmask(dmask, nd[n]);
#pragma unroll
        for (int k = 0; k < S; ++k) v[k] = comp_fixed(fixed, k) ? 0.0 : x[(size_t)nd[n] * S + k];
    }
    // finish = store + sum: the element vector into LDS, stage[a][c][thread], entry by entry through put (i = a SV + c; the select: a
    // skipped element may hold NaN), and the tile's node sums into the partials
    __device__ __forceinline__ void put(double* stage, int i, double v) const { stage[i * TS + tid] = live ? v : 0.0; }
    template <int SV>
    __device__ __forceinline__ void store(const double (&f)[N][SV], double* stage) const {
#pragma unroll
        for (int n = 0; n < N; ++n)
#pragma unroll
            for (int c = 0; c < SV; ++c) put(stage, n * SV + c, f[n][c]);
    }
    template <int SV>
    __device__ __forceinline__ void sum(const VecTiles& t, const double* stage, unsigned short* ents, double* partial) {
        ts.template sum<SV>(t, tile, tid, stage, ents, partial);
    }
    template <int SV>
    __device__ __forceinline__ void finish(const VecTiles& t, const double (&f)[N][SV], double* stage, unsigned short* ents, double* partial) {
        store(f, stage);
        sum<SV>(t, stage, ents, partial);
    }
};

// v summed over the workgroup in the fixed tree of block_sum_256 (xor-shuffles over the lanes, then (w0 + w1) + (w2 + w3)), stored by
// thread 0 as the workgroup's partial.  Whether a kernel leaves a partial at all is its own condition, uniform over the workgroup.
__device__ __forceinline__ void block_partial_store(double v, double* partial) {
    __shared__ double red[4];
    const double tot = block_sum_256(v, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// EX (here and in the tile kernels below): the per-element expansion of a.theta (material.hpp, Stretch) -- the nodal values the body takes are
// U' and its result is scaled on the way out; the body itself is the same.  EX = false is the kernel as it was: the launchers pick it while
// no field is set.
template <int EK, int OP, int TS, int MONO = 0, bool EX = false>
__global__ void __launch_bounds__(TS) k_element_pass_tiled(const KArgs a, const VecTiles t, const unsigned char* active, double* partial) {
    constexpr int N = EPDims<EK, OP, EP_VECTOR>::N, S = EPDims<EK, OP, EP_VECTOR>::S, D = EPDims<EK, OP, EP_VECTOR>::D;
    __shared__ double stage[N * S * TS];
    __shared__ unsigned short ents[(N % 4 == 0) ? TS * N : 4];
    TilePass<N, TS> tp;
    if (!tp.begin(t, active)) return;
    if (a.ablate & 128) {   // (profiling: what the scattered gathers cost -- every thread reads the nodes of its wavefront's first element: wrong results)
#pragma unroll
        for (int n = 0; n < N; ++n) tp.nd[n] = __builtin_amdgcn_readfirstlane(tp.nd[n]);
    }
    double X[N][D], Uv[N][S];
#pragma unroll
    for (int n = 0; n < N; ++n) {
        tp.coords(n, a.verts, X[n]);
        tp.field(n, a.u, Uv[n]);
    }
    // (measured and dropped, Hex8 elasticity 216^3, element pass 1.03 ms: the distinct nodes' coordinates and u through LDS instead of
    // the gathers -- two more barriers, nothing in flight across them: 1.35 ms; u parked in LDS and 168 registers for a third
    // wavefront per SIMD -- 62 registers spill: 1.66 ms)
    double f[N][S];
    double energy;
    if constexpr (EX) {
        const Stretch<OP, D> st = element_stretch<OP, D>(a, tp.ec);
        stretch_nodes<OP, D, N>(st, X, Uv);
        element_pass_body<EK, OP, EP_VECTOR, MONO>(a, tp.el, tp.live, tp.ec, X, EPRegU<N, S>{Uv}, f, energy);
        stretch_scale<OP, D>(st.sP, f);
    } else {
        element_pass_body<EK, OP, EP_VECTOR, MONO>(a, tp.el, tp.live, tp.ec, X, EPRegU<N, S>{Uv}, f, energy);
    }
    tp.store(f, stage);
    if (a.ablate & 64) return;   // (profiling: the element phase alone)
    tp.template sum<S>(t, stage, ents, partial);
}

// energy (compute_element_elliptic_energy, local/elliptic.rs:551-605) over the same tiles: on a numbering without locality the tile order
// is what makes the gathers of the coordinates and of u local; the tile's elements are summed in a fixed tree, one partial per workgroup
// (workgroups beyond the last tile write a zero), k_sum_partials adds them in index order
template <int EK, int OP, int TS, int MONO = 0, bool EX = false>
__global__ void __launch_bounds__(TS) k_element_energy_tiled(const KArgs a, const VecTiles t, const unsigned char* active, double* partial) {
    constexpr int N = EPDims<EK, OP, EP_SCALAR>::N, S = EPDims<EK, OP, EP_SCALAR>::S, D = EPDims<EK, OP, EP_SCALAR>::D;
    static_assert(TS == 256, "the workgroup's sum is a tree over 256 threads");
    TilePass<N, TS, false> tp;
    if (!tp.begin(t, active)) {
        if (threadIdx.x == 0) partial[blockIdx.x] = 0.0;
        return;
    }
    double X[N][D], Uv[N][S];
#pragma unroll
    for (int n = 0; n < N; ++n) {
        tp.coords(n, a.verts, X[n]);
        tp.field(n, a.u, Uv[n]);
    }
    double f[1][S];
    double energy;
    if constexpr (EX) {
        const Stretch<OP, D> st = element_stretch<OP, D>(a, tp.ec);
        stretch_nodes<OP, D, N>(st, X, Uv);
        element_pass_body<EK, OP, EP_SCALAR, MONO>(a, tp.el, tp.live, tp.ec, X, EPRegU<N, S>{Uv}, f, energy);
        energy *= st.sPsi;
    } else {
        element_pass_body<EK, OP, EP_SCALAR, MONO>(a, tp.el, tp.live, tp.ec, X, EPRegU<N, S>{Uv}, f, energy);
    }
    block_partial_store(tp.live ? energy : 0.0, partial);
}

// source vector (local/source.rs:159-278) over the same tiles: source_element_body per thread, the tile's node sums, partials
template <int D, int S, int N, bool FACT, int TS>
__global__ void __launch_bounds__(TS) k_source_elements_tiled(const KArgs a, const SourceG g, const double* values, const VecTiles t,
                                                               const unsigned char* active, double* partial) {
    constexpr int SF = FACT ? 1 : S;
    __shared__ double stage[N * SF * TS];
    __shared__ unsigned short ents[(N % 4 == 0) ? TS * N : 4];
    TilePass<N, TS> tp;
    if (!tp.begin(t, active)) return;
    double X[N][D], f[N][SF];
#pragma unroll
    for (int n = 0; n < N; ++n) tp.coords(n, a.verts, X[n]);
    source_element_body<D, S, N, FACT>(a, g, values, tp.ec, X, f);
    tp.finish(t, f, stage, ents, partial);
}

// The partials of one node summed in ascending order, the only walk over np_off and np_idx: four partials requested before the first sum,
// the additions stay in order (a last group of fewer than four reads the list's last index again and does not add it).  NA arrays of
// partials over the same list, their loads in flight together; an array after the first may be null and sums to zero.
template <int NA, int S>
__device__ __forceinline__ void node_partials_sum(const unsigned* np_off, const unsigned* np_idx, const double* const (&part)[NA], int node,
                                                  double (&acc)[NA][S]) {
#pragma unroll
    for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int c = 0; c < S; ++c) acc[a][c] = 0.0;
    const unsigned k0 = np_off[node], k1 = np_off[node + 1];
    for (unsigned kb = k0; kb < k1; kb += 4) {
        unsigned v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = np_idx[min(kb + j, k1 - 1)];
        double x[4][S][NA];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < S; ++c)
#pragma unroll
                for (int a = 0; a < NA; ++a) x[j][c][a] = (a == 0 || part[a]) ? part[a][(size_t)v[j] * S + c] : 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (kb + j < k1) {
#pragma unroll
                for (int c = 0; c < S; ++c)
#pragma unroll
                    for (int a = 0; a < NA; ++a) acc[a][c] += x[j][c][a];
            }
    }
}
// ... of one array
template <int S>
__device__ __forceinline__ void node_partials_sum(const unsigned* np_off, const unsigned* np_idx, const double* part, int node, double (&acc)[S]) {
    node_partials_sum(np_off, np_idx, {part}, node, reinterpret_cast<double(&)[1][S]>(acc));
}

// SO > 0: the partials are scalars (S = 1) and the node's SO components are  g[c] sum  (k_source_elements_tiled<FACT>)
template <int S, int SO = 0>
__global__ void __launch_bounds__(256) k_vector_from_partials(int num_nodes, const unsigned* np_off, const unsigned* np_idx, const double* partial,
                                                              double* out, const SourceG g = SourceG{{0.0, 0.0, 0.0}}) {
    static_assert(SO == 0 || S == 1, "scaled node sum: scalar partials");
    const int node = blockIdx.x * 256 + threadIdx.x;
    if (node >= num_nodes) return;
    constexpr int SP = SO > 0 ? SO : S;
    double acc[S], prev[SP];
#pragma unroll
    for (int c = 0; c < SP; ++c) prev[c] = out[(size_t)node * SP + c];   // (requested before the sum: the load overlaps it)
    node_partials_sum<S>(np_off, np_idx, partial, node, acc);
    if constexpr (SO > 0) {
#pragma unroll
        for (int c = 0; c < SO; ++c) out[(size_t)node * SO + c] = fma(g.v[c], acc[0], prev[c]);
    } else {
#pragma unroll
        for (int c = 0; c < S; ++c) out[(size_t)node * S + c] = prev[c] + acc[c];
    }
}

// diagonal of the matrix-free map over the tiles (diagonal_element_body for the linear operators; tangent_diagonal_body, with u gathered
// (a.u, may be null: zero), for the nonlinear ones): the tile's node sums, partials; k_vector_from_partials adds them
// (EX: the nonlinear operators only -- the diagonal of a linear operator does not see the field)
template <int EK, int OP, int TS, bool EX = false>
__global__ void __launch_bounds__(TS) k_diagonal_tiled(const KArgs a, const VecTiles t, const unsigned char* active, double* partial) {
    constexpr int N = EPDims<EK, OP, EP_VECTOR>::N, S = EPDims<EK, OP, EP_VECTOR>::S, D = EPDims<EK, OP, EP_VECTOR>::D;
    constexpr bool lin = OP <= FH_LINEAR_ELASTIC;
    __shared__ double stage[N * S * TS];
    __shared__ unsigned short ents[(N % 4 == 0) ? TS * N : 4];
    TilePass<N, TS> tp;
    if (!tp.begin(t, active)) return;
    double X[N][D], Uv[lin ? 1 : N][S], f[N][S];
#pragma unroll
    for (int n = 0; n < N; ++n) {
        tp.coords(n, a.verts, X[n]);
        if constexpr (!lin) tp.field(n, a.u, Uv[n]);
    }
    static_assert(!(EX && lin), "the diagonal of a linear operator does not see the expansion");
    if constexpr (lin) {
        diagonal_element_body<D, S, N, OP>(a, tp.ec, tp.live, X, f);
    } else if constexpr (EX) {
        const Stretch<OP, D> st = element_stretch<OP, D>(a, tp.ec);
        stretch_nodes<OP, D, N>(st, X, Uv);
        tangent_diagonal_body<D, S, N, OP>(a, tp.ec, tp.live, X, Uv, f);
        stretch_scale<OP, D>(st.sT, f);
    } else {
        tangent_diagonal_body<D, S, N, OP>(a, tp.ec, tp.live, X, Uv, f);
    }
    // (finish, with the loops of store written out here: through store, whose loops are unrolled before they meet the body's, f is kept as
    // one vector across the point loop and Tri3 StVK takes 98 registers for 92, four waves per SIMD for five)
#pragma unroll
    for (int n = 0; n < N; ++n)
#pragma unroll
        for (int c = 0; c < S; ++c) tp.put(stage, n * S + c, f[n][c]);
    tp.template sum<S>(t, stage, ents, partial);
}

// tangent of the residual T(u) x of the nonlinear operators over the tiles (matrix-free, engine_vector.hip): the element pass with both u
// (a.u, may be null: zero) and the operand x gathered per element; MONO = 1 / 2: Hex8 in the monomial basis (2: every element affine).  The
// tile's node sums, partials; k_operator_from_partials overwrites y with them.
template <int EK, int OP, int TS, int MONO = 0, bool EX = false>
__global__ void __launch_bounds__(TS) k_tangent_tiled(const KArgs a, const VecTiles t, const unsigned char* active, const double* x, double* partial) {
    constexpr int N = EPDims<EK, OP, EP_VECTOR>::N, S = EPDims<EK, OP, EP_VECTOR>::S, D = EPDims<EK, OP, EP_VECTOR>::D;
    __shared__ double stage[N * S * TS];
    __shared__ unsigned short ents[(N % 4 == 0) ? TS * N : 4];
    TilePass<N, TS> tp;
    if (!tp.begin(t, active)) return;
    double X[N][D], Uv[N][S], Vv[N][S], f[N][S];
#pragma unroll
    for (int n = 0; n < N; ++n) {
        tp.coords(n, a.verts, X[n]);
        tp.field(n, a.u, Uv[n]);
        tp.field_masked(n, x, nullptr, Vv[n]);   // (the operand: always there)
    }
    double sT = 1.0;
    if constexpr (EX) {   // (u alone is strained: the operand enters dP linearly and takes the factor with the result)
        const Stretch<OP, D> st = element_stretch<OP, D>(a, tp.ec);
        stretch_nodes<OP, D, N>(st, X, Uv);
        sT = st.sT;
    }
    if constexpr (MONO != 0 && EK == FH_HEX8) tangent_body_hex8<OP, MONO == 2>(a, tp.ec, tp.live, X, Uv, Vv, f);
    else tangent_element_body<D, S, N, OP>(a, tp.ec, tp.live, X, Uv, Vv, f);
    if constexpr (EX) stretch_scale<OP, D>(sT, f);
    tp.finish(t, f, stage, ents, partial);
}

// element pass of a central-difference step with Rayleigh stiffness damping (engine_dynamics.hip): r(u) + eta_k T(u) v in ONE launch and one
// array of partials, v (the handle's v_h, or v_0 for a_0; its Dirichlet entries are zero) gathered beside u.  Linear operators: r is linear
// and T(u) = A, so the residual's body runs once on u + eta_k v -- no second body, no second gather of X.  Nonlinear operators: the residual's
// body, whose element vector is parked in the thread's own places of the staging array, then the tangent's body on the same X and u, and
// f + eta_k g goes back to those places: the live registers are those of k_tangent_tiled, not of both bodies at once.  MONO as
// k_element_pass_tiled's (form 3 exists for the linear operators only, where the tangent's body is not run).
template <int EK, int OP, int TS, int MONO = 0, bool EX = false>
__global__ void __launch_bounds__(TS) k_damped_pass_tiled(const KArgs a, const VecTiles t, const unsigned char* active, const double* v, double eta_k,
                                                           double* partial) {
    constexpr int N = EPDims<EK, OP, EP_VECTOR>::N, S = EPDims<EK, OP, EP_VECTOR>::S, D = EPDims<EK, OP, EP_VECTOR>::D;
    __shared__ double stage[N * S * TS];
    __shared__ unsigned short ents[(N % 4 == 0) ? TS * N : 4];
    TilePass<N, TS> tp;
    if (!tp.begin(t, active)) return;
    double X[N][D], Uv[N][S], Vv[N][S], f[N][S], energy;
#pragma unroll
    for (int n = 0; n < N; ++n) {
        tp.coords(n, a.verts, X[n]);
        tp.field(n, a.u, Uv[n]);
        tp.field_masked(n, v, nullptr, Vv[n]);   // (the handle's velocity: always there)
    }
    if constexpr (OP <= FH_LINEAR_ELASTIC) {
#pragma unroll
        for (int n = 0; n < N; ++n)
#pragma unroll
            for (int k = 0; k < S; ++k) Uv[n][k] = fma(eta_k, Vv[n][k], Uv[n][k]);
        // (EX: r is affine in u with the same tangent, so r(u) + eta_k A v is the strained body on u + eta_k v as well)
        if constexpr (EX) stretch_nodes<OP, D, N>(element_stretch<OP, D>(a, tp.ec), X, Uv);
        element_pass_body<EK, OP, EP_VECTOR, MONO>(a, tp.el, tp.live, tp.ec, X, EPRegU<N, S>{Uv}, f, energy);
        tp.store(f, stage);
    } else {
        double sP = 1.0, sT = 1.0;
        if constexpr (EX) {
            const Stretch<OP, D> st = element_stretch<OP, D>(a, tp.ec);
            stretch_nodes<OP, D, N>(st, X, Uv);
            sP = st.sP;
            sT = st.sT;
        }
        element_pass_body<EK, OP, EP_VECTOR, MONO>(a, tp.el, tp.live, tp.ec, X, EPRegU<N, S>{Uv}, f, energy);
        if constexpr (EX) stretch_scale<OP, D>(sP, f);
        tp.store(f, stage);
        if constexpr (MONO != 0 && EK == FH_HEX8) tangent_body_hex8<OP, MONO == 2>(a, tp.ec, tp.live, X, Uv, Vv, f);
        else tangent_element_body<D, S, N, OP>(a, tp.ec, tp.live, X, Uv, Vv, f);
        if constexpr (EX) stretch_scale<OP, D>(sT, f);
#pragma unroll
        for (int n = 0; n < N; ++n)
#pragma unroll
            for (int c = 0; c < S; ++c) tp.put(stage, n * S + c, fma(eta_k, f[n][c], stage[(n * S + c) * TS + tp.tid]));
    }
    tp.template sum<S>(t, stage, ents, partial);
}

// node pass of the matrix-free operator y = A x: y[S node + c] = sum of the node's partials in ascending order, OVERWRITTEN (not added).
// dmask (may be null): homogeneous Dirichlet nodes, whose rows hold  scale x  (the element pass saw x with those entries zeroed, so
// their columns are zero already); the element pass saw x 2^-e (xbits: mf_exponent), the sums are scaled back.  dot_partial (may be null): per workgroup  x . y  over its nodes, in a fixed tree.
// ct (count 0: off): the penalty contact term of the node, contact_scale (B + H) x with the UNSCALED x (contact_kernels.hpp; H: the friction
// block, while ct.friction is set, here and in the node passes below the friction force q beside g), joins the scaled-back
// sum before the Dirichlet rows and the dot product are formed; S == 1 has no such term.  G (here and in the three node passes below):
// whether the table may hold a sampled grid (ct.grids); the launches pick G = false while none stands, an instantiation without the grid
// branch and its registers (contact_eval).  A, likewise: whether multipliers stand (ct.mult); with A = false the shift by s_oi and its
// load are not compiled (contact_visit), and the launches pick that instantiation while none stand.
template <int S, bool G, bool A>
__global__ void __launch_bounds__(256) k_operator_from_partials(int num_nodes, const unsigned* np_off, const unsigned* np_idx, const double* partial,
                                                                const double* x, const unsigned char* dmask, const double* scale,
                                                                const unsigned long long* xbits, double* y, double* dot_partial,
                                                                const ContactTable ct, double contact_scale) {
    const int node = blockIdx.x * 256 + threadIdx.x;
    const int ex = mf_exponent(xbits);
    double dot = 0.0;
    if (node < num_nodes) {
        double acc[S];
        node_partials_sum<S>(np_off, np_idx, partial, node, acc);
        const unsigned fixed = node_dmask(dmask, node);
        double xv[S], xo[S];   // (xo: the operand as the element pass saw it, the held components zero, so that their columns of the contact block vanish too)
#pragma unroll
        for (int c = 0; c < S; ++c) {
            xv[c] = x[(size_t)node * S + c];
            xo[c] = comp_fixed(fixed, c) ? 0.0 : xv[c];
            acc[c] = ldexp(acc[c], ex);
        }
        if constexpr (S > 1) {
            if (ct.count) contact_apply<S, G, A>(ct, node, xo, contact_scale, acc);   // (the unscaled operand)
            if (ct.friction) friction_apply<S, G, A>(ct, node, xo, contact_scale, acc);
        }
#pragma unroll
        for (int c = 0; c < S; ++c) {
            const double yv = comp_fixed(fixed, c) ? *scale * xv[c] : acc[c];
            y[(size_t)node * S + c] = yv;
            dot = fma(xv[c], yv, dot);
        }
    }
    if (dot_partial) block_partial_store(dot, dot_partial);
}

// the mass term of the shifted map alpha M + beta T(u) (engine_vector.hip) over the tiles: the element pass of mass_element_body (x null: the
// diagonal) with the operand gathered per element, the entries of the Dirichlet nodes (dmask, may be null) read as zero; the tile's node sums,
// partials.  A pass of its own: the tangent's element passes stay as they are.
template <int D, int N, int S, bool DIAG, int TS>
__global__ void __launch_bounds__(TS) k_mass_tiled(const KArgs a, const VecTiles t, const unsigned char* active, const double* rho, int rho_per_elem,
                                                   const double* x, const unsigned char* dmask, double* partial) {
    __shared__ double stage[N * S * TS];
    __shared__ unsigned short ents[(N % 4 == 0) ? TS * N : 4];
    TilePass<N, TS> tp;
    if (!tp.begin(t, active)) return;
    double X[N][D], Vv[DIAG ? 1 : N][S], f[N][S];
#pragma unroll
    for (int n = 0; n < N; ++n) {
        tp.coords(n, a.verts, X[n]);
        if constexpr (!DIAG) tp.field_masked(n, x, dmask, Vv[n]);
    }
    const double r = rho[rho_per_elem ? tp.ec : 0];
    mass_element_body<D, S, N, N, DIAG>(a, r, X, [&](int n, int k) { return Vv[DIAG ? 0 : n][k]; }, f);
    tp.finish(t, f, stage, ents, partial);
}

// the shifted map fused on Hex8 (the monomial form of element_pass.hpp, MASS instantiations): one element pass forms
// beta T(u) x + alpha M x into the partials, k_operator_from_partials sums them.  Linear operators: the residual's body fed the operand
// (a.u = x, scaled like the operator's); AFFM as k_element_pass_tiled's MONO - 1.
template <int OP, int TS, int AFFM>
__global__ void __launch_bounds__(TS) k_shifted_pass_tiled(const KArgs a, const VecTiles t, const unsigned char* active, const MassTerm mt, double* partial) {
    constexpr int N = 8, S = OpT<OP, 3>::S, D = 3;
    __shared__ double stage[N * S * TS];
    __shared__ unsigned short ents[TS * N];
    TilePass<N, TS> tp;
    if (!tp.begin(t, active)) return;
    double X[N][D], Uv[N][S], f[N][S], energy;
#pragma unroll
    for (int n = 0; n < N; ++n) {
        tp.coords(n, a.verts, X[n]);
        tp.field_masked(n, a.u, nullptr, Uv[n]);   // (the operand: always there)
    }
    element_pass_body_hex8<OP, EP_VECTOR, AFFM, EPRegU<N, S>, true>(a, tp.el, tp.live, tp.ec, X, EPRegU<N, S>{Uv}, f, energy, mt);
    tp.finish(t, f, stage, ents, partial);
}

// ... the nonlinear operators: tangent_body_hex8 with the mass term (x: the tangent's operand)
// (EX: u is strained and the stiffness part takes theta^(d-2) through the element's beta; the mass term is the mass of the reference volume)
template <int OP, int TS, bool AFF, bool EX = false>
__global__ void __launch_bounds__(TS) k_shifted_tangent_tiled(const KArgs a, const VecTiles t, const unsigned char* active, const double* x, const MassTerm mt,
                                                             double* partial) {
    constexpr int N = 8, S = 3, D = 3;
    __shared__ double stage[N * S * TS];
    __shared__ unsigned short ents[TS * N];
    TilePass<N, TS> tp;
    if (!tp.begin(t, active)) return;
    double X[N][D], Uv[N][S], Vv[N][S], f[N][S];
#pragma unroll
    for (int n = 0; n < N; ++n) {
        tp.coords(n, a.verts, X[n]);
        tp.field(n, a.u, Uv[n]);
        tp.field_masked(n, x, nullptr, Vv[n]);   // (the operand: always there)
    }
    if constexpr (EX) {
        const Stretch<OP, D> st = element_stretch<OP, D>(a, tp.ec);
        stretch_nodes<OP, D, N>(st, X, Uv);
        MassTerm me = mt;
        me.beta *= st.sT;
        tangent_body_hex8<OP, AFF, true>(a, tp.ec, tp.live, X, Uv, Vv, f, me);
    } else {
        tangent_body_hex8<OP, AFF, true>(a, tp.ec, tp.live, X, Uv, Vv, f, mt);
    }
    tp.finish(t, f, stage, ents, partial);
}

// ... and the mass alone (beta == 0: u is not read): x with the Dirichlet entries (dmask, may be null) read as zero
template <int S, int TS, bool AFF>
__global__ void __launch_bounds__(TS) k_mass_hex8_tiled(const KArgs a, const VecTiles t, const unsigned char* active, const double* x,
                                                       const unsigned char* dmask, const MassTerm mt, double* partial) {
    constexpr int N = 8, D = 3;
    __shared__ double stage[N * S * TS];
    __shared__ unsigned short ents[TS * N];
    TilePass<N, TS> tp;
    if (!tp.begin(t, active)) return;
    double X[N][D], Vv[N][S], f[N][S];
#pragma unroll
    for (int n = 0; n < N; ++n) {
        tp.coords(n, a.verts, X[n]);
        tp.field_masked(n, x, dmask, Vv[n]);
    }
    mass_body_hex8<S, AFF>(a, tp.ec, X, Vv, mt, f);
    tp.finish(t, f, stage, ents, partial);
}

// node pass of the shifted map: y = alpha (node sums of the mass partials, in ascending order) + beta t, OVERWRITTEN (t: the tangent's y,
// may be y itself, or null = zero); rows of the Dirichlet nodes (dmask, may be null) = *scale x; dot_partial (may be null): per workgroup
// x . y over its nodes in a fixed tree (k_operator_from_partials' layout)
template <int S>
__global__ void __launch_bounds__(256) k_shift_from_partials(int num_nodes, const unsigned* np_off, const unsigned* np_idx, const double* partial,
                                                             const double* x, const unsigned char* dmask, const double* scale, double alpha,
                                                             double beta, const double* tv, double* y, double* dot_partial) {
    const int node = blockIdx.x * 256 + threadIdx.x;
    double dot = 0.0;
    if (node < num_nodes) {
        double acc[S];
        node_partials_sum<S>(np_off, np_idx, partial, node, acc);
        const unsigned fixed = node_dmask(dmask, node);
#pragma unroll
        for (int c = 0; c < S; ++c) {
            const size_t i = (size_t)node * S + c;
            const double xv = x[i], m = alpha * acc[c];
            const double yv = comp_fixed(fixed, c) ? *scale * xv : (tv ? fma(beta, tv[i], m) : m);
            y[i] = yv;
            dot = fma(xv, yv, dot);
        }
    }
    if (dot_partial) block_partial_store(dot, dot_partial);
}

// node pass of the Newton residual (engine_newton.hip): F = alpha (node sums of the mass partials of d = u - u_ref) + beta (node sums of the
// residual partials - f), OVERWRITTEN, both sums in ascending order and over one walk of the node's list, so that their loads are in flight
// together (mpart null: alpha = 0; f null: zero);
// rows of the Dirichlet nodes (dmask, may be null) are zero.  norm_partial: per workgroup |F|^2 over its nodes, in a fixed tree
// (k_operator_from_partials' layout), summed in index order by the caller.  ct (count 0: off): the contact force g of the node
// (contact_kernels.hpp) joins the residual sum first, so F and |F|^2 are those of r + g.
template <int S, bool G, bool A>
__global__ void __launch_bounds__(256) k_newton_from_partials(int num_nodes, const unsigned* np_off, const unsigned* np_idx, const double* rpart,
                                                              const double* mpart, const double* f, const unsigned char* dmask, double alpha,
                                                              double beta, double* F, double* norm_partial, const ContactTable ct) {
    const int node = blockIdx.x * 256 + threadIdx.x;
    double sq = 0.0;
    if (node < num_nodes) {
        double acc[2][S];
        node_partials_sum(np_off, np_idx, {rpart, mpart}, node, acc);
        double(&racc)[S] = acc[0], (&macc)[S] = acc[1];
        const unsigned fixed = node_dmask(dmask, node);
        if constexpr (S > 1) {
            if (ct.count) contact_force<S, G, A>(ct, node, racc);
            if (ct.friction) friction_force<S, G, A>(ct, node, racc);
        }
#pragma unroll
        for (int c = 0; c < S; ++c) {
            const size_t i = (size_t)node * S + c;
            const double r = f ? racc[c] - f[i] : racc[c];
            const double v = comp_fixed(fixed, c) ? 0.0 : (mpart ? fma(beta, r, alpha * macc[c]) : beta * r);
            F[i] = v;
            sq = fma(v, v, sq);
        }
    }
    block_partial_store(sq, norm_partial);
}

// (the arguments beside the table, of every node pass that takes one: contact_kernels.hpp holds table + NODE_PASS_ARG_BYTES under 4 KB)
static_assert(4 * sizeof(void*) + sizeof(DynStep) <= NODE_PASS_ARG_BYTES && 4 * sizeof(void*) + sizeof(FoStage) <= NODE_PASS_ARG_BYTES &&
                  12 * sizeof(void*) <= NODE_PASS_ARG_BYTES,
              "a node pass's own arguments have outgrown the room the contact table leaves them");

// node pass of a central-difference step (engine_dynamics.hip): the node's residual partials summed in ascending order as
// k_vector_from_partials forms them, and in the same visit the integrator's whole state update (dyn_dof, dynamics_kernels.hpp): a_{n+1} =
// (lf f - r) / m, the second kick that completes v_{n+1}, then either the stores and the kinetic-energy partial of a record (DYN_STORE) or
// the next step's first kick and drift into the context's u (DYN_ADVANCE).  The element pass that follows reads the u this leaves.
// ct (count 0: off): the contact force g at the u the element pass read joins r before dyn_dof, which stays as it is.
template <int S, bool G, bool A>
__global__ void __launch_bounds__(256) k_dynamics_from_partials(int num_nodes, const unsigned* np_off, const unsigned* np_idx, const double* rpart,
                                                                const DynStep p, const ContactTable ct) {
    const int node = blockIdx.x * 256 + threadIdx.x;
    double ke = 0.0;
    if (node < num_nodes) {
        double racc[S];
        node_partials_sum<S>(np_off, np_idx, rpart, node, racc);
        if constexpr (S > 1) {
            if (ct.count) contact_force<S, G, A>(ct, node, racc);
            if (ct.friction) friction_force<S, G, A>(ct, node, racc);   // (the slip of the velocity the node is about to kick: ct.slip_v is p.v)
        }
        const unsigned fixed = node_dmask(p.dmask, node);
        const double lf = dyn_load_factor(p);
#pragma unroll
        for (int c = 0; c < S; ++c) ke += dyn_dof(p, (size_t)node * S + c, comp_fixed(fixed, c), lf, racc[c]);
    }
    if (p.flags & DYN_STORE) block_partial_store(ke, p.ke_partial);
}

// node pass of one stage of a first-order Runge-Kutta-Legendre step, or of the rate alone (engine_dynamics.hip): the same ordered sum, then
// fo_dof (dynamics_step.hpp): Y_j from Y_{j-1} (the context's u) and Y_{j-2} (prev), both updated in this visit; with FO_STORE the partial
// of sum m y^2 of the u just written, so a recorded step needs no launch of its own.  The element pass that follows reads the u this leaves.
// ct (count 0: off): the contact force g at Y_{j-1} joins r before fo_dof, which stays as it is.
template <int S, bool G, bool A>
__global__ void __launch_bounds__(256) k_first_order_from_partials(int num_nodes, const unsigned* np_off, const unsigned* np_idx, const double* rpart,
                                                                   const FoStage p, const ContactTable ct) {
    const int node = blockIdx.x * 256 + threadIdx.x;
    double q = 0.0;
    if (node < num_nodes) {
        double racc[S];
        node_partials_sum<S>(np_off, np_idx, rpart, node, racc);
        if constexpr (S > 1) {
            if (ct.count) contact_force<S, G, A>(ct, node, racc);
        }
        const unsigned fixed = node_dmask(p.dmask, node);
        const double lf = dyn_load_factor(p);
#pragma unroll
        for (int c = 0; c < S; ++c) q += fo_dof(p, (size_t)node * S + c, comp_fixed(fixed, c), lf, racc[c]);
    }
    if (p.flags & FO_STORE) block_partial_store(q, p.partial);
}

// the longest run of an offset table, max over i < n of off[i + 1] - off[i] (vector_tiles_stats: formed on request, nothing of it is kept)
__global__ void __launch_bounds__(256) k_vt_longest_run(const unsigned* off, unsigned n, unsigned* out) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) atomicMax(out, off[i + 1] - off[i]);
}

template <typename T>
hipError_t vt_alloc(VecTilesStore* st, int slot, T** p, size_t count) {
    hipError_t e = hipMalloc(reinterpret_cast<void**>(p), sizeof(T) * (count ? count : 1));
    if (e == hipSuccess) st->bufs[slot] = *p;
    return e;
}

}  // namespace

#define VT_TRY(expr)                                  \
    do {                                              \
        const hipError_t vt_e_ = (expr);              \
        if (vt_e_ != hipSuccess) { cleanup(); return vt_e_; } \
    } while (0)

void VecTilesStore::release() {
    for (void*& b : bufs) {
        if (b) (void)hipFree(b);
        b = nullptr;
    }
    v = VecTiles{};
}

hipError_t vector_tiles_build(hipStream_t stream, const int* conn, int n, long long E, const double* verts, int D, int num_nodes, VecTilesStore* out,
                              int* bad) {
    int ts = VT_TS;
    *bad = 0;
    out->release();
    // (the partial sums are counted in 32 bits: at most E n of them)
    if (E <= 0 || n < 1 || n > 8 || D < 1 || D > 3 || num_nodes <= 0 || E > 0x7fffff00ll || (unsigned long long)E * (unsigned)n >= (1ull << 32) - 256) { *bad = 1; return hipSuccess; }
    // (128-element tiles, two wavefronts per workgroup and four workgroups per CU, were measured: 1.33 against 1.28 ms for the residual of Hex8 216^3)
    const int T = (int)((E + ts - 1) / ts);
    void* tmp[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    auto cleanup = [&]() {
        for (void*& p : tmp) {
            if (p) (void)hipFree(p);
            p = nullptr;
        }
    };
    // bounding box of the vertices -> Morton keys of the element centroids
    const int bgrid = 256;
    double* d_box = nullptr;
    VT_TRY(hipMalloc(&tmp[0], sizeof(double) * 6 * bgrid));
    d_box = (double*)tmp[0];
    hipLaunchKernelGGL(k_vt_bbox, dim3(bgrid), dim3(256), 0, stream, verts, num_nodes, D, d_box);
    std::vector<double> h_box(6 * bgrid);
    VT_TRY(hipMemcpyAsync(h_box.data(), d_box, sizeof(double) * 6 * bgrid, hipMemcpyDeviceToHost, stream));
    VT_TRY(hipStreamSynchronize(stream));
    Box3 box;
    for (int i = 0; i < 3; ++i) {
        double lo = 1e300, hi = -1e300;
        for (int b = 0; b < bgrid; ++b) { lo = std::min(lo, h_box[6 * b + i]); hi = std::max(hi, h_box[6 * b + 3 + i]); }
        box.lo[i] = lo;
        box.scale[i] = hi > lo ? 2097151.0 / (hi - lo) : 0.0;
    }
    unsigned long long *k_in = nullptr, *k_out = nullptr;
    int *v_in = nullptr, *v_out = nullptr, *d_bad = nullptr;
    VT_TRY(hipMalloc(&tmp[1], sizeof(unsigned long long) * E)); k_in = (unsigned long long*)tmp[1];
    VT_TRY(hipMalloc(&tmp[2], sizeof(unsigned long long) * E)); k_out = (unsigned long long*)tmp[2];
    VT_TRY(hipMalloc(&tmp[3], sizeof(int) * E)); v_in = (int*)tmp[3];
    VT_TRY(hipMalloc(&tmp[4], sizeof(int) * E)); v_out = (int*)tmp[4];
    VT_TRY(hipMalloc(&tmp[5], sizeof(int) * 4)); d_bad = (int*)tmp[5];
    VT_TRY(hipMemsetAsync(d_bad, 0, sizeof(int) * 4, stream));
    hipLaunchKernelGGL(k_vt_morton, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, stream, conn, n, E, verts, D, num_nodes, box, k_in, v_in, d_bad);
    size_t sort_bytes = 0;
    VT_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, k_in, k_out, v_in, v_out, (int)E, 0, 63, stream));
    VT_TRY(hipMalloc(&tmp[6], sort_bytes + 16));
    VT_TRY(hipcub::DeviceRadixSort::SortPairs(tmp[6], sort_bytes, k_in, k_out, v_in, v_out, (int)E, 0, 63, stream));
    int h_bad = 0;
    VT_TRY(hipMemcpyAsync(&h_bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, stream));
    VT_TRY(hipStreamSynchronize(stream));
    if (h_bad) { cleanup(); *bad = 1; return hipSuccess; }
    // keys are done: their buffers hold the tile counts and offsets
    unsigned* tile_cnt = (unsigned*)k_in;     // T + 1 <= E + 1 entries of 4 bytes fit (E >= 1: 8 bytes per key)
    int* elem = nullptr;
    unsigned* noff = nullptr;
    if (vt_alloc(out, 0, &elem, (size_t)T * ts) != hipSuccess || vt_alloc(out, 1, &noff, (size_t)T + 1) != hipSuccess) { cleanup(); out->release(); return hipErrorOutOfMemory; }
    if ((size_t)(T + 1) * sizeof(unsigned) > sizeof(unsigned long long) * (size_t)E) {   // (tiny meshes)
        (void)hipFree(tmp[1]); tmp[1] = nullptr;
        VT_TRY(hipMalloc(&tmp[1], sizeof(unsigned) * ((size_t)T + 1)));
        tile_cnt = (unsigned*)tmp[1];
    }
    VT_TRY(hipMemsetAsync(tile_cnt, 0, sizeof(unsigned) * ((size_t)T + 1), stream));
    hipLaunchKernelGGL((k_vt_tile_tables<false, VT_TS>), dim3(T), dim3(VT_TS), 0, stream, v_out, E, conn, n, tile_cnt, (const unsigned*)nullptr, (int*)nullptr,
                       (int*)nullptr, (unsigned short*)nullptr, (unsigned short*)nullptr, (unsigned*)nullptr);
    size_t scan_bytes = 0;
    VT_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, tile_cnt, noff, T + 1, stream));
    if (scan_bytes + 16 > sort_bytes + 16) {
        (void)hipFree(tmp[6]); tmp[6] = nullptr;
        VT_TRY(hipMalloc(&tmp[6], scan_bytes + 16));
    }
    VT_TRY(hipcub::DeviceScan::ExclusiveSum(tmp[6], scan_bytes, tile_cnt, noff, T + 1, stream));
    unsigned P = 0;
    VT_TRY(hipMemcpyAsync(&P, noff + T, sizeof(unsigned), hipMemcpyDeviceToHost, stream));
    VT_TRY(hipStreamSynchronize(stream));
    // (more than 2^32 partials would have wrapped the scan: E n < 2^32 is checked by the caller's flat_len; P <= E n)
    unsigned short *la_off = nullptr, *la = nullptr;
    int* tconn = nullptr;
    unsigned *np_off = nullptr, *np_idx = nullptr, *p_node = nullptr;
    hipError_t e = vt_alloc(out, 2, &tconn, (size_t)T * n * ts);
    if (e == hipSuccess) e = vt_alloc(out, 3, &la_off, (size_t)P + T + 1);
    if (e == hipSuccess) e = vt_alloc(out, 4, &la, (size_t)T * n * ts);
    if (e == hipSuccess) e = vt_alloc(out, 5, &np_off, (size_t)num_nodes + 1);
    if (e == hipSuccess) e = vt_alloc(out, 6, &np_idx, (size_t)P);
    if (e != hipSuccess) { cleanup(); out->release(); return e; }
    if (vt_alloc(out, 7, &p_node, (size_t)P + 1) != hipSuccess) { cleanup(); out->release(); return hipErrorOutOfMemory; }
    (void)hipFree(tmp[2]); tmp[2] = nullptr;
    hipLaunchKernelGGL((k_vt_tile_tables<true, VT_TS>), dim3(T), dim3(VT_TS), 0, stream, v_out, E, conn, n, tile_cnt, (const unsigned*)noff, elem, tconn, la_off, la, p_node);
    // node -> partials
    unsigned *deg = nullptr, *cursor = nullptr;
    VT_TRY(hipMalloc(&tmp[7], sizeof(unsigned) * 2 * ((size_t)num_nodes + 1)));
    deg = (unsigned*)tmp[7];
    cursor = deg + num_nodes + 1;
    VT_TRY(hipMemsetAsync(deg, 0, sizeof(unsigned) * 2 * ((size_t)num_nodes + 1), stream));
    if (P) hipLaunchKernelGGL(k_vt_count, dim3((P + 255) / 256), dim3(256), 0, stream, p_node, P, deg);
    VT_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, deg, np_off, num_nodes + 1, stream));
    (void)hipFree(tmp[6]); tmp[6] = nullptr;
    VT_TRY(hipMalloc(&tmp[6], scan_bytes + 16));
    VT_TRY(hipcub::DeviceScan::ExclusiveSum(tmp[6], scan_bytes, deg, np_off, num_nodes + 1, stream));
    if (P) {
        hipLaunchKernelGGL(k_vt_fill, dim3((P + 255) / 256), dim3(256), 0, stream, p_node, P, np_off, cursor, np_idx);
        hipLaunchKernelGGL(k_vt_sort_lists, dim3((num_nodes + 255) / 256), dim3(256), 0, stream, np_off, np_idx, num_nodes);
    }
    VT_TRY(hipStreamSynchronize(stream));
    VT_TRY(hipGetLastError());
    cleanup();
    out->v = VecTiles{elem, tconn, noff, la_off, la, np_off, np_idx, p_node, T, n, P, ts};
    return hipSuccess;
}

hipError_t vector_tiles_stats(hipStream_t stream, const VecTiles& t, int num_nodes, unsigned* max_tile_nodes, unsigned* max_node_partials) {
    unsigned* d = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d), sizeof(unsigned) * 2);
    if (e != hipSuccess) return e;
    unsigned h[2] = {0u, 0u};
    e = hipMemsetAsync(d, 0, sizeof(unsigned) * 2, stream);
    if (e == hipSuccess) {
        if (t.ntiles > 0) hipLaunchKernelGGL(k_vt_longest_run, dim3((t.ntiles + 255) / 256), dim3(256), 0, stream, t.noff, (unsigned)t.ntiles, d);
        if (num_nodes > 0) hipLaunchKernelGGL(k_vt_longest_run, dim3((num_nodes + 255) / 256), dim3(256), 0, stream, t.np_off, (unsigned)num_nodes, d + 1);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h, d, sizeof(unsigned) * 2, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    (void)hipFree(d);
    *max_tile_nodes = h[0];
    *max_node_partials = h[1];
    return e;
}

// ---- the launchers.  An element pass returns -1 where the combination has no kernel (the callers keep their other kernels).
namespace {
// an element pass: one workgroup per tile, in whole groups of eight (xcd_tile); a node pass: `grid` workgroups of 256
template <class... P, class... A>
int tile_launch(void (*kern)(P...), const VecTiles& t, hipStream_t stream, const A&... args) {
    hipLaunchKernelGGL(kern, dim3(8 * ((t.ntiles + 7) / 8)), dim3(VT_TS), 0, stream, args...);
    return 0;
}
template <class... P, class... A>
hipError_t node_launch(void (*kern)(P...), int grid, hipStream_t stream, const A&... args) {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, stream, args...);
    return hipGetLastError();
}
// The form of the element pass (element_pass.hpp): 0 general; Hex8 with the table of monomials: 1, 2 when every element is affine, 3 when the
// rule's moments are there too (the linear operators only)
int mono_mode(int elem_kind, int op, const KArgs& a) {
    if (elem_kind != FH_HEX8 || !a.qmono) return 0;
    if (!a.all_affine) return 1;
    return (a.qmom && op <= FH_LINEAR_ELASTIC) ? 3 : 2;
}
constexpr bool mono_has_kernel(int ek, int op, int mode) { return mode == 0 || (ek == FH_HEX8 && (mode < 3 || op <= FH_LINEAR_ELASTIC)); }
// f(element kind, operator, form) for a low-order kind, an operator of `ops` and the form the arguments ask for
// ... and with or without the expansion (a.theta; an operator without such a kernel: -1, the host has refused it before)
template <int... OPs, class F>
int dispatch_tile_pass(int elem_kind, int_list<OPs...> ops, int op, const KArgs& a, F&& f) {
    return dispatch(low_order_kinds, elem_kind, ops, op, -1, [&](auto ek, auto opc) {
        return dispatch(int_list<0, 1, 2, 3>{}, mono_mode(elem_kind, op, a), -1, [&](auto m) {
            return dispatch_bool(a.theta != nullptr, [&](auto ex) {
                if constexpr (mono_has_kernel(ek(), opc(), m()) && (!ex() || op_expands(opc()))) return f(ek, opc, m, ex);
                else return -1;
            });
        });
    });
}
}  // namespace

int vector_tiles_element_pass(int elem_kind, int op, hipStream_t stream, const KArgs& a, const VecTiles& t, const unsigned char* active, double* partial) {
    return dispatch_tile_pass(elem_kind, elliptic_ops, op, a, [&](auto ek, auto opc, auto m, auto ex) {
        return tile_launch(k_element_pass_tiled<ek(), opc(), VT_TS, m(), ex()>, t, stream, a, t, active, partial);
    });
}

int vector_tiles_damped_pass(int elem_kind, int op, hipStream_t stream, const KArgs& a, const VecTiles& t, const unsigned char* active, const double* v,
                             double eta_k, double* partial) {
    return dispatch_tile_pass(elem_kind, elliptic_ops, op, a, [&](auto ek, auto opc, auto m, auto ex) {
        return tile_launch(k_damped_pass_tiled<ek(), opc(), VT_TS, m(), ex()>, t, stream, a, t, active, v, eta_k, partial);
    });
}

int vector_tiles_energy_pass(int elem_kind, int op, hipStream_t stream, const KArgs& a, const VecTiles& t, const unsigned char* active, double* partial) {
    return dispatch_tile_pass(elem_kind, elliptic_ops, op, a, [&](auto ek, auto opc, auto m, auto ex) {
        tile_launch(k_element_energy_tiled<ek(), opc(), VT_TS, m(), ex()>, t, stream, a, t, active, partial);
        return vector_tiles_energy_partials(t);   // one partial per workgroup
    });
}

int vector_tiles_source_pass(int D, int sdim, int n, bool fact, hipStream_t stream, const KArgs& a, const double* g3, const double* values,
                             const VecTiles& t, const unsigned char* active, double* partial) {
    SourceG g{{g3 ? g3[0] : 0.0, g3 ? g3[1] : 0.0, g3 ? g3[2] : 0.0}};
    // the low-order kinds by (D, n): simplex or cube; one component, or (any other sdim) D of them
    return dispatch(int_list<2, 3>{}, D, int_list<3, 4, 8>{}, n, -1, [&](auto dc, auto nc) {
        if constexpr (nc() != dc() + 1 && nc() != (1 << dc())) return -1;
        else return dispatch_bool(sdim == 1, [&](auto scalar) {
            return dispatch_bool(fact, [&](auto fc) {
                return tile_launch(k_source_elements_tiled<dc(), scalar() ? 1 : dc(), nc(), fc(), VT_TS>, t, stream, a, g, values, t, active, partial);
            });
        });
    });
}

hipError_t vector_tiles_node_pass(hipStream_t stream, int S, int num_nodes, const VecTiles& t, const double* partial, double* out, const double* scaled_g) {
    const int grid = (num_nodes + 255) / 256;
    return dispatch_or_last(solution_dims, S, [&](auto s) {
        if (!scaled_g) return node_launch(k_vector_from_partials<s(), 0>, grid, stream, num_nodes, t.np_off, t.np_idx, partial, out, SourceG{});
        const SourceG g{{scaled_g[0], scaled_g[1], scaled_g[2]}};   // scalar partials, S components g[c] sum
        return node_launch(k_vector_from_partials<1, s()>, grid, stream, num_nodes, t.np_off, t.np_idx, partial, out, g);
    });
}

int vector_tiles_diagonal_pass(int elem_kind, int op, hipStream_t stream, const KArgs& a, const VecTiles& t, const unsigned char* active, double* partial) {
    return dispatch(low_order_kinds, elem_kind, elliptic_ops, op, -1, [&](auto ek, auto opc) {
        if constexpr (op_depends_on_u(opc()))
            return dispatch_bool(a.theta != nullptr, [&](auto ex) {
                return tile_launch(k_diagonal_tiled<ek(), opc(), VT_TS, ex()>, t, stream, a, t, active, partial);
            });
        else
            return tile_launch(k_diagonal_tiled<ek(), opc(), VT_TS>, t, stream, a, t, active, partial);
    });
}

// the two compile-time flags of the node passes that take the table: G (a grid stands; without: the instantiation without the grid branch)
// and A (multipliers stand; without: the instantiation without the shift by s_oi)
template <class F>
static auto dispatch_contact_flags(const ContactTable& ct, F&& f) {
    return dispatch_bool(ct.grids != 0, [&](auto g) { return dispatch_bool(ct.mult != nullptr, [&](auto m) { return f(g, m); }); });
}

hipError_t vector_tiles_operator_node_pass(hipStream_t stream, int S, int num_nodes, const VecTiles& t, const double* partial, const double* x,
                                           const unsigned char* dmask, const double* scale, const unsigned long long* xbits, double* y,
                                           double* dot_partial, const ContactTable& ct, double contact_scale) {
    return dispatch_or_last(solution_dims, S, [&](auto s) {
        return dispatch_contact_flags(ct, [&](auto g, auto m) {
            return node_launch(k_operator_from_partials<s(), g(), m()>, vector_tiles_operator_partials(num_nodes), stream, num_nodes, t.np_off, t.np_idx, partial, x, dmask,
                           scale, xbits, y, dot_partial, ct, contact_scale);
        });
    });
}

int vector_tiles_tangent_pass(int elem_kind, int op, hipStream_t stream, const KArgs& a, const VecTiles& t, const unsigned char* active, const double* x,
                              double* partial) {
    return dispatch_tile_pass(elem_kind, hyperelastic_ops, op, a, [&](auto ek, auto opc, auto m, auto ex) {
        return tile_launch(k_tangent_tiled<ek(), opc(), VT_TS, m(), ex()>, t, stream, a, t, active, x, partial);
    });
}

int vector_tiles_mass_pass(int elem_kind, int S, hipStream_t stream, const KArgs& a, const VecTiles& t, const unsigned char* active, const double* rho,
                           int rho_per_elem, const double* x, const unsigned char* dmask, double* partial) {
    return dispatch(low_order_kinds, elem_kind, -1, [&](auto ek) {
        constexpr int D = kind_geom<ek()>::D, N = kind_geom<ek()>::NG;   // (iso-parametric: N == NG)
        if (S != 1 && S != D) return -1;
        return dispatch_bool(S == 1, [&](auto scalar) {
            return dispatch_bool(x == nullptr, [&](auto diag) {   // no operand: the diagonal
                return tile_launch(k_mass_tiled<D, N, scalar() ? 1 : D, diag(), VT_TS>, t, stream, a, t, active, rho, rho_per_elem, x, dmask, partial);
            });
        });
    });
}

hipError_t vector_tiles_shift_node_pass(hipStream_t stream, int S, int num_nodes, const VecTiles& t, const double* partial, const double* x,
                                        const unsigned char* dmask, const double* scale, double alpha, double beta, const double* tv, double* y,
                                        double* dot_partial) {
    return dispatch_or_last(solution_dims, S, [&](auto s) {
        return node_launch(k_shift_from_partials<s()>, vector_tiles_operator_partials(num_nodes), stream, num_nodes, t.np_off, t.np_idx, partial, x, dmask,
                           scale, alpha, beta, tv, y, dot_partial);
    });
}

hipError_t vector_tiles_newton_node_pass(hipStream_t stream, int S, int num_nodes, const VecTiles& t, const double* rpart, const double* mpart,
                                         const double* f, const unsigned char* dmask, double alpha, double beta, double* F, double* norm_partial,
                                         const ContactTable& ct) {
    return dispatch_or_last(solution_dims, S, [&](auto s) {
        return dispatch_contact_flags(ct, [&](auto g, auto m) {
            return node_launch(k_newton_from_partials<s(), g(), m()>, vector_tiles_operator_partials(num_nodes), stream, num_nodes, t.np_off, t.np_idx, rpart, mpart, f,
                           dmask, alpha, beta, F, norm_partial, ct);
        });
    });
}

hipError_t vector_tiles_dynamics_node_pass(hipStream_t stream, int S, int num_nodes, const VecTiles& t, const double* rpart, const DynStep& p,
                                           const ContactTable& ct) {
    return dispatch_or_last(solution_dims, S, [&](auto s) {
        return dispatch_contact_flags(ct, [&](auto g, auto m) {
            return node_launch(k_dynamics_from_partials<s(), g(), m()>, vector_tiles_operator_partials(num_nodes), stream, num_nodes, t.np_off, t.np_idx, rpart, p, ct);
        });
    });
}

hipError_t vector_tiles_first_order_node_pass(hipStream_t stream, int S, int num_nodes, const VecTiles& t, const double* rpart, const FoStage& p,
                                              const ContactTable& ct) {
    return dispatch_or_last(solution_dims, S, [&](auto s) {
        return dispatch_contact_flags(ct, [&](auto g, auto m) {
            return node_launch(k_first_order_from_partials<s(), g(), m()>, vector_tiles_operator_partials(num_nodes), stream, num_nodes, t.np_off, t.np_idx, rpart, p, ct);
        });
    });
}

int vector_tiles_shifted_hex8_pass(int op, hipStream_t stream, const KArgs& a, const VecTiles& t, const unsigned char* active, const double* x,
                                   const unsigned char* dmask, const MassTerm& mt, double* partial) {
    if (!a.qmono) return -1;
    const bool aff = a.all_affine != 0;
    if (mt.beta == 0.0)   // the mass alone: any operator but FH_LAPLACE has three components
        return dispatch_bool(op == FH_LAPLACE, [&](auto scalar) {
            return dispatch_bool(aff, [&](auto affc) {
                return tile_launch(k_mass_hex8_tiled<scalar() ? 1 : 3, VT_TS, affc()>, t, stream, a, t, active, x, dmask, mt, partial);
            });
        });
    return dispatch(elliptic_ops, op, -1, [&](auto opc) {
        if constexpr (opc() <= FH_LINEAR_ELASTIC)   // form 0 general, 1 affine, 2 affine with the rule's moments
            return dispatch(int_list<0, 1, 2>{}, !aff ? 0 : a.qmom ? 2 : 1, -1, [&](auto m) {
                return tile_launch(k_shifted_pass_tiled<opc(), VT_TS, m()>, t, stream, a, t, active, mt, partial);
            });
        else
            return dispatch_bool(aff, [&](auto affc) {
                return dispatch_bool(a.theta != nullptr, [&](auto ex) {
                    return tile_launch(k_shifted_tangent_tiled<opc(), VT_TS, affc(), ex()>, t, stream, a, t, active, x, mt, partial);
                });
            });
    });
}

}  // namespace fenris_hip
