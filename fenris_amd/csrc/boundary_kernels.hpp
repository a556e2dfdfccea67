#pragma once
// Boundary-face search and surface-load kernels (engine_boundary.hip).  Integer work only in the search: no floating point, no atomics.
#include <hip/hip_runtime.h>

namespace fenris_hip {

// Local faces of a cell kind: `nfaces` faces of `nfn` nodes each, in the order and ORIENTATION (outward) of the reference's
// get_face_connectivity (src/connectivity.rs; the tables are filled in engine_boundary.hip with the lines they restate).  By value in
// the kernel arguments.
struct FaceTable {
    int nfaces, nfn;
    signed char nodes[6][9];
};

// The sorted node tuple of face `fid` = cell * nfaces + local face: the identity of a face (src/mesh.rs:173-181).  Odd-even transposition
// with compile-time indices: the tuple stays in registers.
template <int NFN>
__device__ __forceinline__ void face_sorted_tuple(const int* __restrict__ conn, int n, const FaceTable& t, unsigned fid, unsigned (&k)[NFN]) {
    const unsigned cell = fid / (unsigned)t.nfaces, lf = fid % (unsigned)t.nfaces;
    const int* ec = conn + (size_t)cell * n;
#pragma unroll
    for (int a = 0; a < NFN; ++a) k[a] = (unsigned)ec[t.nodes[lf][a]];
#pragma unroll
    for (int pass = 0; pass < NFN; ++pass) {
#pragma unroll
        for (int i = pass & 1; i + 1 < NFN; i += 2) {
            const unsigned lo = min(k[i], k[i + 1]), hi = max(k[i], k[i + 1]);
            k[i] = lo;
            k[i + 1] = hi;
        }
    }
}

// -1 / 0 / 1: lexicographic order of two sorted tuples
template <int NFN>
__device__ __forceinline__ int face_tuple_cmp(const unsigned (&a)[NFN], const unsigned (&b)[NFN]) {
    int r = 0;
#pragma unroll
    for (int i = NFN - 1; i >= 0; --i) r = (a[i] < b[i]) ? -1 : (a[i] > b[i]) ? 1 : r;
    return r;
}

// Stage 1: the sort key of every (cell, local face): its two smallest nodes, `bits` bits each, the smallest in the high half -- the
// bucket of the face.  The value is the face id.
template <int NFN>
__global__ void k_face_keys(const int* __restrict__ conn, int n, FaceTable t, unsigned nf_all, int bits, unsigned long long* __restrict__ keys,
                            unsigned* __restrict__ vals) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nf_all) return;
    unsigned k[NFN];
    face_sorted_tuple<NFN>(conn, n, t, i, k);
    keys[i] = ((unsigned long long)k[0] << bits) | (unsigned long long)k[1];
    vals[i] = i;
}

// Stage 3 (after the sort by key): a face is a boundary face iff no other face of its bucket has the same FULL tuple (mesh.rs:187-200:
// the count of the tuple is exactly one; three cells on one face are not boundary either).
template <int NFN>
__global__ void k_face_unique(const int* __restrict__ conn, int n, FaceTable t, unsigned nf_all, const unsigned long long* __restrict__ keys,
                              const unsigned* __restrict__ vals, unsigned* __restrict__ flag) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nf_all) return;
    const unsigned long long key = keys[i];
    unsigned mine[NFN], other[NFN];
    bool twin = false;
    if (NFN > 2) face_sorted_tuple<NFN>(conn, n, t, vals[i], mine);
    for (long long j = (long long)i - 1; j >= 0 && !twin && keys[j] == key; --j) {
        if (NFN == 2) { twin = true; break; }   // the key is the whole tuple
        face_sorted_tuple<NFN>(conn, n, t, vals[j], other);
        twin = face_tuple_cmp<NFN>(mine, other) == 0;
    }
    for (long long j = (long long)i + 1; j < (long long)nf_all && !twin && keys[j] == key; ++j) {
        if (NFN == 2) { twin = true; break; }
        face_sorted_tuple<NFN>(conn, n, t, vals[j], other);
        twin = face_tuple_cmp<NFN>(mine, other) == 0;
    }
    flag[i] = twin ? 0u : 1u;
}

// Stage 5: the boundary faces in ascending lexicographic order of their sorted tuples (the BTreeMap iteration, mesh.rs:197-202): the
// buckets are in key order, `scan` counts the boundary faces in front of a bucket, and inside its bucket a face ranks itself by full
// compare.  Output: the face's nodes in the cell's orientation, the cell, the local face index.
template <int NFN>
__global__ void k_face_emit(const int* __restrict__ conn, int n, FaceTable t, unsigned nf_all, const unsigned long long* __restrict__ keys,
                            const unsigned* __restrict__ vals, const unsigned* __restrict__ flag, const unsigned* __restrict__ scan,
                            unsigned long long* __restrict__ face_nodes, unsigned long long* __restrict__ cells, unsigned* __restrict__ local_faces) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nf_all || !flag[i]) return;
    const unsigned long long key = keys[i];
    long long first = i;
    while (first > 0 && keys[first - 1] == key) --first;
    unsigned rank = 0;
    if (NFN > 2) {
        unsigned mine[NFN], other[NFN];
        face_sorted_tuple<NFN>(conn, n, t, vals[i], mine);
        for (long long j = first; j < (long long)nf_all && keys[j] == key; ++j) {
            if (j == (long long)i || !flag[j]) continue;
            face_sorted_tuple<NFN>(conn, n, t, vals[j], other);
            rank += face_tuple_cmp<NFN>(other, mine) < 0 ? 1u : 0u;
        }
    }
    const size_t pos = (size_t)scan[first] + rank;
    const unsigned fid = vals[i], cell = fid / (unsigned)t.nfaces, lf = fid % (unsigned)t.nfaces;
    const int* ec = conn + (size_t)cell * n;
#pragma unroll
    for (int a = 0; a < NFN; ++a) face_nodes[pos * NFN + a] = (unsigned long long)ec[t.nodes[lf][a]];
    cells[pos] = cell;
    local_faces[pos] = lf;
}

// membership flags of a u64 id list (boundary vertices / cells): every writer stores the same value
__global__ void k_mark_ids(const unsigned long long* __restrict__ ids, size_t count, unsigned* __restrict__ flag) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) flag[ids[i]] = 1u;
}
__global__ void k_compact_flagged(const unsigned* __restrict__ flag, const unsigned* __restrict__ scan, size_t domain, unsigned long long* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < domain && flag[i]) out[scan[i]] = i;
}

// ---- surface load ----------------------------------------------------------------------------------------------------------------
// One record per (local face, face point): everything that depends on the reference element only, tabulated on the host with the
// engine's ref_basis / ref_gradients at the face point mapped into the cell (engine_boundary.hip).
//   G[a][k]   gradient of the geometry basis of corner a (the sub-parametric corner map: hexahedron.rs:324-330 and kin)
//   PG[a]     its value (for the physical point)
//   NF[m]     the cell's basis function of face node m
//   nref[k]   d phi/ds x d phi/dt of the face-to-cell map phi (2D: the tangent turned clockwise): reference normal times reference measure
struct FacePointRec {
    double G[8][3];
    double PG[8];
    double NF[9];
    double nref[3];
};

struct SurfaceArgs {
    const double* verts;
    const int* conn;
    const unsigned long long* cells;
    const unsigned* local_faces;
    unsigned long long num_faces, E;
    int n, nq, sdim, pressure;   // n: nodes per cell
    const double* w;             // nq
    const FacePointRec* recs;    // nfaces x nq
    const double* data;          // traction: sdim per item, pressure: 1 per item
    int data_mode;               // 0: one item, 1: one per face, 2: one per (face, point)
    double* out;
};

// a_q = cof(J) nref with J = sum_a X_a G_a^T: Nanson's det(J) J^-T n without the division, so a degenerate face gives a zero vector
template <int D, int NG>
__device__ __forceinline__ void face_area_vector(const double (&X)[NG][D], const FacePointRec& r, double (&av)[D]) {
    double J[D][D];
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int k = 0; k < D; ++k) {
            double s = 0.0;
#pragma unroll
            for (int a = 0; a < NG; ++a) s += X[a][i] * r.G[a][k];
            J[i][k] = s;
        }
    if constexpr (D == 2) {
        av[0] = J[1][1] * r.nref[0] - J[1][0] * r.nref[1];
        av[1] = -J[0][1] * r.nref[0] + J[0][0] * r.nref[1];
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
                s += (J[i1][k1] * J[i2][k2] - J[i1][k2] * J[i2][k1]) * r.nref[k];
            }
            av[i] = s;
        }
    }
}

template <int D, int NG>
__device__ __forceinline__ void face_load_corners(const SurfaceArgs& a, unsigned long long cell, double (&X)[NG][D]) {
    const int* ec = a.conn + (size_t)cell * a.n;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const size_t v = (size_t)ec[g];
#pragma unroll
        for (int i = 0; i < D; ++i) X[g][i] = a.verts[v * D + i];
    }
}

// One thread per node of the face list: the entries (node, position * nfn + face node) are sorted by node with the positions ascending,
// the thread at the head of a node's run walks it and adds the node's sum to out -- ascending (position, q), no atomics.
template <int D, int NG>
__global__ void k_surface_load(SurfaceArgs a, int nfn, const unsigned* __restrict__ ent_node, const unsigned* __restrict__ ent, size_t num_entries) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_entries) return;
    const unsigned node = ent_node[i];
    if (i > 0 && ent_node[i - 1] == node) return;
    double acc[3] = {0.0, 0.0, 0.0};
    for (size_t j = i; j < num_entries && ent_node[j] == node; ++j) {
        const unsigned long long pos = ent[j] / (unsigned)nfn;
        const int m = (int)(ent[j] % (unsigned)nfn);
        const unsigned long long cell = a.cells[pos];
        const unsigned lf = a.local_faces[pos];
        double X[NG][D];
        face_load_corners<D, NG>(a, cell, X);
        for (int q = 0; q < a.nq; ++q) {
            const FacePointRec& r = a.recs[(size_t)lf * a.nq + q];
            double av[D];
            face_area_vector<D, NG>(X, r, av);
            const double wn = a.w[q] * r.NF[m];
            const size_t item = a.data_mode == 0 ? 0 : a.data_mode == 1 ? (size_t)pos : (size_t)pos * a.nq + q;
            if (a.pressure) {
                const double p = a.data[item];
#pragma unroll
                for (int c = 0; c < D; ++c) acc[c] += -wn * p * av[c];
            } else {
                double m2 = 0.0;
#pragma unroll
                for (int c = 0; c < D; ++c) m2 += av[c] * av[c];
                const double ds = sqrt(m2);
                if (a.sdim == 1) acc[0] += wn * a.data[item] * ds;
                else {
#pragma unroll
                    for (int c = 0; c < D; ++c) acc[c] += wn * a.data[item * D + c] * ds;
                }
            }
        }
    }
    if (a.sdim == 1) a.out[node] += acc[0];
    else {
#pragma unroll
        for (int c = 0; c < D; ++c) a.out[(size_t)node * D + c] += acc[c];
    }
}

// the entries of the adjacency, and the check of the list: a cell or local face out of range sets *bad and emits node 0
__global__ void k_surface_entries(const int* __restrict__ conn, int n, FaceTable t, const unsigned long long* __restrict__ cells,
                                  const unsigned* __restrict__ local_faces, unsigned long long num_faces, unsigned long long E,
                                  unsigned* __restrict__ ent_node, unsigned* __restrict__ ent, int* __restrict__ bad) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_faces * (size_t)t.nfn) return;
    const size_t pos = i / t.nfn;
    const int m = (int)(i % t.nfn);
    const unsigned long long cell = cells[pos];
    const unsigned lf = local_faces[pos];
    ent[i] = (unsigned)i;
    if (cell >= E || lf >= (unsigned)t.nfaces) { *bad = 1; ent_node[i] = 0u; return; }
    ent_node[i] = (unsigned)conn[(size_t)cell * n + t.nodes[lf][m]];
}

// a fingerprint of the face list, the key of the cached adjacency: a sum of mixed words (order of the sum does not matter for integers)
__global__ void k_surface_list_hash(const unsigned long long* __restrict__ cells, const unsigned* __restrict__ local_faces, unsigned long long num_faces,
                                    unsigned long long* __restrict__ h) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_faces) return;
    unsigned long long x = cells[i] * 8ull + local_faces[i] + 0x9E3779B97F4A7C15ull * (i + 1);
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;   // splitmix64 finaliser
    h[i] = x;
}

// x_q of every (face, point): the corner map at the face point (map_reference_coords of the cell)
template <int D, int NG>
__global__ void k_face_physical_points(SurfaceArgs a, double* __restrict__ x) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.num_faces * (size_t)a.nq) return;
    const size_t pos = i / a.nq;
    const int q = (int)(i % a.nq);
    const unsigned long long cell = a.cells[pos];
    const unsigned lf = a.local_faces[pos];
    double X[NG][D];
    face_load_corners<D, NG>(a, cell, X);
    const FacePointRec& r = a.recs[(size_t)lf * a.nq + q];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        double s = 0.0;
#pragma unroll
        for (int g = 0; g < NG; ++g) s += X[g][k] * r.PG[g];
        x[i * D + k] = s;
    }
}

}  // namespace fenris_hip
