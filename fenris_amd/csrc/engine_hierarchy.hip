// The passes that derive a mesh from the context's mesh on the device, each with a CSR transfer, and hold the result on the context
// (DESIGN.md section 3.6.3):
//   uniform refinement   fh_refine_uniform   what fh_refine_hex8_uniform does on the host for Hex8; the reference's refine_uniformly,
//                                            src/mesh/refinement.rs, covers Tri3 (3.6.3a)
//   degree coarsening    fh_coarsen_degree   the linear mesh on the vertex nodes of a Tet10, Tri6, Quad9, Hex20 or Hex27 mesh (3.6.3b)
//   degree elevation     fh_elevate_degree   the quadratic mesh over a linear one, numbered and placed bit for bit as
//                                            fh_refine_to_quadratic and fh_hex8_to_hex27 do on the host, host_inputs.cpp (3.6.3c)
// One store type holds any of the three results and one set of accessors serves them; refinement and elevation label their new nodes
// through one core (label_candidates).  The coarsening uses no sort (owner / flags / check / scan) and shares the store alone.
#include "engine_internal.hpp"
#include "refine_kernels.hpp"
#include "coarsen_kernels.hpp"
#include "elevate_kernels.hpp"

#include <memory>

// ---- the held result: a derived mesh and its transfer (CSR by the nodes of the finer side), on the device
struct HeldMesh {
    int elem_kind = -1, d = 0, n = 0;   // of the derived mesh; n: nodes per cell
    uint64_t num_vertices = 0, num_cells = 0, num_rows = 0, nnz = 0;   // num_rows: the rows of the transfer
    DevBuf<double> verts, weights;
    DevBuf<unsigned long long> conn, offsets, indices;
    DevBuf<unsigned long long> vertex_nodes;   // degree coarsening alone: the node of the high mesh under every vertex
};

extern "C++" void held_drop_all(fh_ctx* c) {
    for (HeldMesh*& h : c->held) {
        delete h;
        h = nullptr;
    }
}

namespace {

// what the messages call a slot's result, and the call that forms it
constexpr const char* held_what[HELD_SLOTS] = {"refinement", "degree coarsening", "degree elevation"};
constexpr const char* held_maker[HELD_SLOTS] = {"fh_refine_uniform", "fh_coarsen_degree", "fh_elevate_degree"};

void held_replace(fh_ctx* c, HeldSlot slot, std::unique_ptr<HeldMesh>& r) {
    delete c->held[slot];
    c->held[slot] = r.release();
}

int held_check(fh_ctx* c, HeldSlot slot, const char* who) {
    if (!c->held[slot])
        return c->fail(FH_INVALID_STATE, std::string(who) + ": no " + held_what[slot] + " held (" + held_maker[slot] + "; fh_set_mesh* drops it)");
    return FH_OK;
}

int held_mesh(fh_ctx* c, HeldSlot slot, const char* who, double* vertices, uint64_t* connectivity, uint64_t* vertex_nodes) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int rc = held_check(c, slot, who);
    if (rc) return rc;
    const HeldMesh* r = c->held[slot];
    if (vertices && r->num_vertices)
        HIP_TRY(c, hipMemcpyAsync(vertices, r->verts.p, sizeof(double) * r->num_vertices * r->d, hipMemcpyDeviceToHost, c->stream));
    if (connectivity && r->num_cells)
        HIP_TRY(c, hipMemcpyAsync(connectivity, r->conn.p, sizeof(uint64_t) * r->num_cells * r->n, hipMemcpyDeviceToHost, c->stream));
    if (vertex_nodes && r->num_vertices)
        HIP_TRY(c, hipMemcpyAsync(vertex_nodes, r->vertex_nodes.p, sizeof(uint64_t) * r->num_vertices, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FH_OK;
}

int held_transfer(fh_ctx* c, HeldSlot slot, const char* who, uint64_t* offsets, uint64_t* indices, double* weights) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int rc = held_check(c, slot, who);
    if (rc) return rc;
    const HeldMesh* r = c->held[slot];
    if (offsets) HIP_TRY(c, hipMemcpyAsync(offsets, r->offsets.p, sizeof(uint64_t) * (r->num_rows + 1), hipMemcpyDeviceToHost, c->stream));
    if (indices && r->nnz) HIP_TRY(c, hipMemcpyAsync(indices, r->indices.p, sizeof(uint64_t) * r->nnz, hipMemcpyDeviceToHost, c->stream));
    if (weights && r->nnz) HIP_TRY(c, hipMemcpyAsync(weights, r->weights.p, sizeof(double) * r->nnz, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FH_OK;
}

// the mesh `from` holds in `slot` becomes the mesh of `to`, device to device
int held_hand_over(fh_ctx* to, fh_ctx* from, HeldSlot slot, const char* who) {
    if (!to || !from) return FH_BAD_ARGUMENT;
    if (held_check(from, slot, who)) return to->fail(FH_INVALID_STATE, from->err);
    if (to->device != from->device) return to->fail(FH_BAD_ARGUMENT, std::string(who) + ": the two contexts are on different devices");
    // fh_set_mesh_dev drops what its context holds: taken off the giving context for the call, so that to == from works
    HeldMesh* r = from->held[slot];
    from->held[slot] = nullptr;
    {
        DevGuard dev_guard_(from->device);
        (void)hipStreamSynchronize(from->stream);   // (the result was formed on the giving context's stream)
    }
    const int rc = fh_set_mesh_dev(to, r->elem_kind, r->verts.p, r->num_vertices, reinterpret_cast<const uint64_t*>(r->conn.p), r->num_cells);
    if (to == from) delete r;
    else from->held[slot] = r;
    return rc;
}

// ---- the parent tables

// Tet10 / Tri6: the edges of ref_basis (engine_internal.hpp; tetrahedron.rs:179-195, triangle.rs:211-224)
CoarsenTable simplex_table(int n, int nv, const int (*edges)[2]) {
    CoarsenTable t{};
    t.n = n; t.nv = nv;
    for (int l = 0; l < nv; ++l) { t.cnt[l] = 1; t.par[l][0] = (signed char)l; }
    for (int l = nv; l < n; ++l) {
        t.cnt[l] = 2;
        t.par[l][0] = (signed char)edges[l - nv][0];
        t.par[l][1] = (signed char)edges[l - nv][1];
    }
    return t;
}
// Quad9 / Hex20 / Hex27: a node's parents are the corners that agree with its reference position on its nonzero axes, in ascending local
// node (QUAD9_SIGN, HEX_SIGN: the tables the basis functions are built from)
template <int D, class Sign>
CoarsenTable lattice_table(int n, int nv, const Sign& sign) {
    CoarsenTable t{};
    t.n = n; t.nv = nv;
    for (int l = 0; l < n; ++l) {
        int cnt = 0;
        for (int a = 0; a < nv; ++a) {
            bool ok = true;
            for (int r = 0; r < D; ++r) ok = ok && (sign[l][r] == 0.0 || sign[a][r] == sign[l][r]);
            if (ok) t.par[l][cnt++] = (signed char)a;
        }
        t.cnt[l] = (signed char)cnt;
    }
    return t;
}

}  // namespace

// the table and the linear kind; false for a kind without a degree coarsening
bool fenris_hip::coarsen_table(int kind, CoarsenTable& t, int& linear_kind) {
    static const int E3[6][2] = {{0, 1}, {1, 2}, {0, 2}, {0, 3}, {2, 3}, {1, 3}};
    static const int E2[3][2] = {{0, 1}, {1, 2}, {0, 2}};
    switch (kind) {
        case FH_TET10: t = simplex_table(10, 4, E3); linear_kind = FH_TET4; return true;
        case FH_TRI6: t = simplex_table(6, 3, E2); linear_kind = FH_TRI3; return true;
        case FH_QUAD9: t = lattice_table<2>(9, 4, QUAD9_SIGN); linear_kind = FH_QUAD4; return true;
        case FH_HEX20: t = lattice_table<3>(20, 8, HEX_SIGN); linear_kind = FH_HEX8; return true;
        case FH_HEX27: t = lattice_table<3>(27, 8, HEX_SIGN); linear_kind = FH_HEX8; return true;
        default: return false;
    }
}

namespace {

constexpr int_list<2, 4, 8> tuple_sizes{};   // the most parents of a node: the tuple lengths with an instantiation

// the labelled slots of t from s0 on, all but `unmatched` of them through the sort
LabelTable label_table(const CoarsenTable& t, int s0, int unmatched, int keep) {
    LabelTable l{};
    l.t = t;
    l.s0 = s0;
    l.S = t.n - s0;
    l.Sm = l.S - unmatched;
    l.keep = keep;
    return l;
}

// The new points and the children of a refinement.  Tet4, Tri3 and Quad4 split at the nodes their quadratic kind adds, so their new
// points are that kind's table: local index n + p of a child names local node n + p of the Tet10, Tri6 or Quad9.  Every new point goes
// through the sort, the centre of a Quad4 or Hex8 included: a Hex8's centre is not the last point of its lattice.
//   Tet4   Bey's red refinement, the inner octahedron cut along (0,2)-(1,3), nodes 1 and 3 of the two inner children that Bey's own
//          order leaves negatively oriented swapped.  All eight children have the parent's orientation and 1/8 of its volume, and
//          repeated refinement stays within 3 congruence classes: any other choice of swaps does not.
//   Tri3   detail.rs:116-127 with d, e, f = 3, 4, 5
//   Hex8   the 3x3x3 lattice of refine_hex8_uniform (host_inputs.cpp), x fastest, its new points numbered in that order (not the Hex27's
//          node order); a lattice point's parents are the corners that agree with it on its nonzero axes, in ascending local node; child
//          (cx, cy, cz) takes the lattice points (cx, cy, cz) + its nodes' offsets
bool refine_table(int kind, LabelTable& l, RefineChildren& ch) {
    static const signed char TET4[8][8] = {{0, 4, 6, 7}, {4, 1, 5, 9}, {6, 5, 2, 8}, {7, 9, 8, 3}, {4, 6, 7, 9}, {4, 9, 5, 6}, {6, 7, 9, 8}, {6, 8, 9, 5}};
    static const signed char TRI3[8][8] = {{0, 3, 5}, {3, 1, 4}, {5, 4, 2}, {3, 4, 5}};
    static const signed char QUAD4[8][8] = {{0, 4, 8, 7}, {4, 1, 5, 8}, {8, 5, 2, 6}, {7, 8, 6, 3}};
    CoarsenTable t{};
    int linear_kind = -1;
    ch = RefineChildren{};
    const signed char (*children)[8] = nullptr;
    switch (kind) {
        case FH_TET4: coarsen_table(FH_TET10, t, linear_kind); ch.C = 8; children = TET4; break;
        case FH_TRI3: coarsen_table(FH_TRI6, t, linear_kind); ch.C = 4; children = TRI3; break;
        case FH_QUAD4: coarsen_table(FH_QUAD9, t, linear_kind); ch.C = 4; children = QUAD4; break;
        case FH_HEX8: {
            t.nv = 8; t.n = 8;
            int lat[27];
            for (int k = 0; k < 3; ++k)
                for (int j = 0; j < 3; ++j)
                    for (int i = 0; i < 3; ++i) {
                        const int L[3] = {i - 1, j - 1, k - 1};
                        int cnt = 0, par[8];
                        for (int a = 0; a < 8; ++a) {
                            bool ok = true;
                            for (int r = 0; r < 3; ++r) ok = ok && (L[r] == 0 || (int)HEX_SIGN[a][r] == L[r]);
                            if (ok) par[cnt++] = a;
                        }
                        if (cnt == 1) { lat[i + 3 * j + 9 * k] = par[0]; continue; }
                        t.cnt[t.n] = (signed char)cnt;
                        for (int q = 0; q < cnt; ++q) t.par[t.n][q] = (signed char)par[q];
                        lat[i + 3 * j + 9 * k] = t.n++;
                    }
            for (int a = 0; a < 8; ++a) { t.cnt[a] = 1; t.par[a][0] = (signed char)a; }
            ch.C = 8;
            for (int cz = 0; cz < 2; ++cz)
                for (int cy = 0; cy < 2; ++cy)
                    for (int cx = 0; cx < 2; ++cx)
                        for (int a = 0; a < 8; ++a) {
                            const int i = cx + ((int)HEX_SIGN[a][0] + 1) / 2, j = cy + ((int)HEX_SIGN[a][1] + 1) / 2, k = cz + ((int)HEX_SIGN[a][2] + 1) / 2;
                            ch.child[cx + 2 * cy + 4 * cz][a] = (signed char)lat[i + 3 * j + 9 * k];
                        }
            break;
        }
        default: return false;
    }
    if (children) std::memcpy(ch.child, children, sizeof ch.child);
    l = label_table(t, t.nv, 0, 1);
    ch.n = t.nv;
    ch.P = l.S;
    return true;
}

// ---- the labelling core of refinement and elevation (hierarchy_kernels.hpp): keys, stable radix sort, first candidates, scan

// The scratch of a labelling, 24 bytes per candidate (keys and ids, twice each for the sort) and the sort's own, and what it holds when
// label_candidates returns: the unsorted ids the first candidates, the sorted keys the scan; the sorted ids are free.
struct Labelling {
    DevBuf<unsigned long long> keys_in, keys;
    DevBuf<unsigned> ids_in, ids;
    DevBuf<char> tmp;
    uint64_t winners = 0, row_entries = 0;   // the scan's totals: the nodes labelled, the entries of their transfer rows
    const unsigned* first() const { return ids_in.p; }
    const unsigned long long* scan() const { return keys.p; }
};

// Labels the E * t.S candidates of the context's cells (at least one, fewer than 2^31).  `bits` is the width of a vertex index in the
// key: the callers differ in it on purpose, because it sets the sort's passes (an elevation pads the key of a vertex candidate with
// N itself, a refinement has no such candidate).
int label_candidates(fh_ctx* c, const LabelTable& t, int bits, Labelling& L) {
    hipStream_t st = c->stream;
    const unsigned E = (unsigned)c->E;
    const unsigned nlab = E * (unsigned)t.S, nsort = E * (unsigned)t.Sm;
    int mp_matched = 2;
    for (int l = t.s0; l < t.s0 + t.Sm; ++l) mp_matched = std::max(mp_matched, (int)t.t.cnt[l]);
    const int sort_grid = (int)((nsort + 255u) / 256u);
    HIP_TRY(c, L.keys_in.alloc(nlab));
    HIP_TRY(c, L.keys.alloc(nlab));
    HIP_TRY(c, L.ids_in.alloc(nlab));
    HIP_TRY(c, L.ids.alloc(nlab));
    size_t sort_bytes = 0, scan_bytes = 0;
    HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, L.keys_in.p, L.keys.p, L.ids_in.p, L.ids.p, (int)nsort, 0, 2 * bits, st));
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, L.keys_in.p, L.keys.p, (int)nlab, st));
    HIP_TRY(c, L.tmp.alloc(std::max(sort_bytes, scan_bytes)));
    dispatch(tuple_sizes, mp_matched, 0, [&](auto m) {
        hipLaunchKernelGGL(k_label_keys<m()>, dim3(sort_grid), dim3(256), 0, st, c->conn.p, t, nsort, (unsigned)c->N, bits, L.keys_in.p, L.ids_in.p);
        return 0;
    });
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(L.tmp.p, sort_bytes, L.keys_in.p, L.keys.p, L.ids_in.p, L.ids.p, (int)nsort, 0, 2 * bits, st));
    // once sorted, the unsorted keys take the scan's input and the unsorted ids the first candidates; the scan goes over the sorted keys
    unsigned* first = L.ids_in.p;
    unsigned long long* val = L.keys_in.p;
    unsigned long long* scan = L.keys.p;
    dispatch(tuple_sizes, mp_matched, 0, [&](auto m) {
        hipLaunchKernelGGL(k_label_first<m()>, dim3(sort_grid), dim3(256), 0, st, c->conn.p, t, nsort, E, L.keys.p, L.ids.p, first, val);
        return 0;
    });
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(L.tmp.p, scan_bytes, val, scan, (int)nlab, st));
    unsigned long long tail[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(&tail[0], val + (nlab - 1), sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&tail[1], scan + (nlab - 1), sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    const unsigned long long total = tail[0] + tail[1];
    L.winners = total >> LABEL_SHIFT;
    L.row_entries = total & ((1ull << LABEL_SHIFT) - 1);
    return FH_OK;
}

// the buffers of a derived mesh of r->n nodes per cell, once its counts are known
int held_alloc(fh_ctx* c, HeldMesh* r) {
    HIP_TRY(c, r->verts.alloc((size_t)r->num_vertices * r->d));
    HIP_TRY(c, r->conn.alloc((size_t)r->num_cells * r->n));
    HIP_TRY(c, r->offsets.alloc((size_t)r->num_rows + 1));
    HIP_TRY(c, r->indices.alloc((size_t)r->nnz));
    HIP_TRY(c, r->weights.alloc((size_t)r->nnz));
    return FH_OK;
}

// the vertices that keep their indices: their positions and identity rows; thread N closes the offsets
int kept_vertex_rows(fh_ctx* c, HeldMesh* r) {
    const unsigned N = (unsigned)c->N;
    dispatch_or_last(int_list<2, 3>{}, r->d, [&](auto d) {
        hipLaunchKernelGGL(k_refine_coarse_rows<d()>, dim3(N / 256u + 1u), dim3(256), 0, c->stream, c->verts.p, N, (unsigned long long)r->num_vertices,
                           (unsigned long long)r->nnz, r->verts.p, r->offsets.p, r->indices.p, r->weights.p);
        return 0;
    });
    HIP_TRY(c, hipGetLastError());
    return FH_OK;
}

// ---- uniform refinement

int refine_uniform(fh_ctx* c, const LabelTable& t, const RefineChildren& ch) {
    hipStream_t st = c->stream;
    const unsigned N = (unsigned)c->N;
    const uint64_t nocc64 = c->E * (uint64_t)t.S;
    if (nocc64 >= (1ull << 31)) return c->fail(FH_UNSUPPORTED, "fh_refine_uniform: num_elements * new points per cell must be < 2^31");
    const unsigned nocc = (unsigned)nocc64;
    int bits = 1;
    while ((1ull << bits) < c->N) ++bits;
    int mp = 2;
    for (int l = t.s0; l < t.t.n; ++l) mp = std::max(mp, (int)t.t.cnt[l]);
    auto r = std::make_unique<HeldMesh>();
    r->elem_kind = c->elem_kind;
    r->d = c->ei.d;
    r->n = ch.n;
    r->num_cells = c->E * (uint64_t)ch.C;
    Labelling L;
    if (nocc) {
        int rc = label_candidates(c, t, bits, L);
        if (rc) return rc;
    }
    r->num_vertices = r->num_rows = c->N + L.winners;
    r->nnz = c->N + L.row_entries;
    if (r->num_vertices >= (1ull << 31)) return c->fail(FH_UNSUPPORTED, "fh_refine_uniform: the refined mesh must have < 2^31 vertices");
    int rc = held_alloc(c, r.get());
    if (rc) return rc;
    rc = kept_vertex_rows(c, r.get());
    if (rc) return rc;
    if (nocc) {
        const int grid = (int)((nocc + 255u) / 256u);
        unsigned* fine = L.ids.p;   // the per-cell table of fine indices: the children read every entry several times
        hipLaunchKernelGGL(k_refine_fine_index, dim3(grid), dim3(256), 0, st, nocc, N, L.first(), L.scan(), fine);
        HIP_TRY(c, hipGetLastError());
        const unsigned long long total = (unsigned long long)r->num_cells * ch.n;
        hipLaunchKernelGGL(k_refine_children, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, c->conn.p, ch, total, fine, r->conn.p);
        HIP_TRY(c, hipGetLastError());
        dispatch(tuple_sizes, mp, int_list<2, 3>{}, r->d, 0, [&](auto m, auto d) {
            hipLaunchKernelGGL((k_refine_new_rows<m(), d()>), dim3(grid), dim3(256), 0, st, c->verts.p, c->conn.p, t, nocc, N, L.first(), L.scan(),
                               r->verts.p, r->offsets.p, r->indices.p, r->weights.p);
            return 0;
        });
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipStreamSynchronize(st));   // the scratch is released on return
    held_replace(c, HELD_REFINEMENT, r);
    c->last_kernel = "k_label_keys + radix sort + k_label_first + scan + k_refine_fine_index + k_refine_children + k_refine_new_rows";
    return FH_OK;
}

// ---- degree coarsening

int coarsen_degree(fh_ctx* c, const CoarsenTable& t, int linear_kind) {
    hipStream_t st = c->stream;
    const unsigned N = (unsigned)c->N;
    int mp = 1;
    for (int l = 0; l < t.n; ++l) mp = std::max(mp, (int)t.cnt[l]);
    const uint64_t nocc64 = c->E * (uint64_t)t.n;
    if (nocc64 >= (1ull << 31)) return c->fail(FH_UNSUPPORTED, "fh_coarsen_degree: num_elements * nodes per cell must be < 2^31");
    if (c->N * (uint64_t)mp >= (1ull << 31))
        return c->fail(FH_UNSUPPORTED, "fh_coarsen_degree: num_vertices * most parents of a node must be < 2^31");
    const unsigned nocc = (unsigned)nocc64;
    auto r = std::make_unique<HeldMesh>();
    r->elem_kind = linear_kind;
    r->d = c->ei.d;
    r->n = t.nv;
    r->num_cells = c->E;
    r->num_rows = c->N;
    // scratch, 28 bytes per node: owner, role, the scan's input and output, the fine index per coarse vertex
    DevBuf<unsigned> owner, role, vfine, status;
    DevBuf<unsigned long long> val, scan;
    DevBuf<char> tmp;
    HIP_TRY(c, status.alloc(COARSEN_STATUS_WORDS));
    HIP_TRY(c, owner.alloc(N));
    HIP_TRY(c, role.alloc(N));
    HIP_TRY(c, vfine.alloc(N));
    HIP_TRY(c, val.alloc(N));
    HIP_TRY(c, scan.alloc(N));
    const unsigned node_grid = N / 256u + 1u, occ_grid = (nocc + 255u) / 256u;
    hipLaunchKernelGGL(k_coarsen_init, dim3(node_grid), dim3(256), 0, st, N, owner.p, role.p, status.p);
    HIP_TRY(c, hipGetLastError());
    if (nocc) {
        hipLaunchKernelGGL(k_coarsen_owner, dim3(occ_grid), dim3(256), 0, st, c->conn.p, t, nocc, owner.p, role.p);
        HIP_TRY(c, hipGetLastError());
    }
    if (N) {
        hipLaunchKernelGGL(k_coarsen_flags, dim3(node_grid), dim3(256), 0, st, t, N, owner.p, role.p, val.p, status.p);
        HIP_TRY(c, hipGetLastError());
        if (nocc) {
            dispatch(tuple_sizes, mp, 0, [&](auto m) {
                hipLaunchKernelGGL(k_coarsen_check<m()>, dim3(occ_grid), dim3(256), 0, st, c->conn.p, t, nocc, owner.p, status.p);
                return 0;
            });
            HIP_TRY(c, hipGetLastError());
        }
        size_t scan_bytes = 0;
        HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, val.p, scan.p, (int)N, st));
        HIP_TRY(c, tmp.alloc(scan_bytes));
        HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(tmp.p, scan_bytes, val.p, scan.p, (int)N, st));
    }
    // one wait for the validation's verdict and the scan's totals
    unsigned h_status[COARSEN_STATUS_WORDS] = {COARSEN_NONE, COARSEN_NONE, COARSEN_NONE};
    unsigned long long tail[2] = {0, 0};
    if (N) {
        HIP_TRY(c, hipMemcpyAsync(&tail[0], val.p + (N - 1), sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(&tail[1], scan.p + (N - 1), sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(c, hipMemcpyAsync(h_status, status.p, sizeof(h_status), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    const unsigned long long total = tail[0] + tail[1];
    if (h_status[COARSEN_ORPHAN] != COARSEN_NONE)
        return c->fail(FH_BAD_ARGUMENT, "fh_coarsen_degree: node " + std::to_string(h_status[COARSEN_ORPHAN]) + " belongs to no cell");
    if (h_status[COARSEN_MIXED] != COARSEN_NONE)
        return c->fail(FH_BAD_ARGUMENT, "fh_coarsen_degree: node " + std::to_string(h_status[COARSEN_MIXED]) +
                                            " is a vertex of one cell and an edge, face or interior node of another");
    if (h_status[COARSEN_MISMATCH] != COARSEN_NONE)
        return c->fail(FH_BAD_ARGUMENT, "fh_coarsen_degree: node " + std::to_string(h_status[COARSEN_MISMATCH]) +
                                            " lies between different vertices in two cells that share it");
    const unsigned M = (unsigned)(total >> COARSEN_SHIFT);
    r->num_vertices = M;
    r->nnz = total & ((1ull << COARSEN_SHIFT) - 1);
    int rc = held_alloc(c, r.get());
    if (rc) return rc;
    HIP_TRY(c, r->vertex_nodes.alloc(M));
    dispatch(tuple_sizes, mp, 0, [&](auto m) {
        hipLaunchKernelGGL(k_coarsen_rows<m()>, dim3(node_grid), dim3(256), 0, st, c->conn.p, t, N, (unsigned long long)r->nnz, owner.p, scan.p,
                           r->offsets.p, r->indices.p, r->weights.p, vfine.p);
        return 0;
    });
    HIP_TRY(c, hipGetLastError());
    if (nocc) {
        const unsigned long long cells_total = (unsigned long long)r->num_cells * t.nv;
        hipLaunchKernelGGL(k_coarsen_cells, dim3((unsigned)((cells_total + 255) / 256)), dim3(256), 0, st, c->conn.p, t, cells_total, scan.p, r->conn.p);
        HIP_TRY(c, hipGetLastError());
    }
    if (M) {
        dispatch_or_last(int_list<2, 3>{}, r->d, [&](auto d) {
            hipLaunchKernelGGL(k_coarsen_vertices<d()>, dim3((M + 255u) / 256u), dim3(256), 0, st, c->verts.p, M, vfine.p, r->verts.p, r->vertex_nodes.p);
            return 0;
        });
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipStreamSynchronize(st));   // the scratch is released on return
    held_replace(c, HELD_COARSENING, r);
    c->last_kernel = "k_coarsen_owner + k_coarsen_flags + k_coarsen_check + scan + k_coarsen_rows + k_coarsen_cells + k_coarsen_vertices";
    return FH_OK;
}

// ---- degree elevation

int elevate_degree(fh_ctx* c, const LabelTable& t, int to_kind) {
    hipStream_t st = c->stream;
    const int n = t.t.n;
    if (c->E * (uint64_t)n >= (1ull << 31)) return c->fail(FH_UNSUPPORTED, "fh_elevate_degree: num_elements * nodes per high cell must be < 2^31");
    const unsigned nlab = (unsigned)c->E * (unsigned)t.S;
    const unsigned base = t.keep ? (unsigned)c->N : 0u;
    int mp = 2;
    for (int l = t.s0; l < n; ++l) mp = std::max(mp, (int)t.t.cnt[l]);
    int bits = 1;
    while ((1ull << bits) <= c->N) ++bits;   // N itself is the second parent of a vertex candidate
    auto r = std::make_unique<HeldMesh>();
    r->elem_kind = to_kind;
    r->d = c->ei.d;
    r->n = n;
    r->num_cells = c->E;
    Labelling L;
    if (nlab) {
        int rc = label_candidates(c, t, bits, L);
        if (rc) return rc;
    }
    r->num_vertices = r->num_rows = base + L.winners;
    r->nnz = base + L.row_entries;
    if (r->num_vertices >= (1ull << 31)) return c->fail(FH_UNSUPPORTED, "fh_elevate_degree: the high mesh must have < 2^31 nodes");
    int rc = held_alloc(c, r.get());
    if (rc) return rc;
    if (t.keep) {
        rc = kept_vertex_rows(c, r.get());
        if (rc) return rc;
    } else if (!nlab) {
        HIP_TRY(c, hipMemsetAsync(r->offsets.p, 0, sizeof(unsigned long long), st));
    }
    if (nlab) {
        const unsigned long long total = (unsigned long long)r->num_cells * n;
        hipLaunchKernelGGL(k_elevate_cells, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, c->conn.p, t, total, base, L.first(), L.scan(),
                           r->conn.p);
        HIP_TRY(c, hipGetLastError());
        dispatch(tuple_sizes, mp, int_list<2, 3>{}, r->d, 0, [&](auto m, auto d) {
            hipLaunchKernelGGL((k_elevate_rows<m(), d()>), dim3((nlab + 255u) / 256u), dim3(256), 0, st, c->verts.p, c->conn.p, t, nlab, base,
                               (unsigned long long)r->num_vertices, (unsigned long long)r->nnz, L.first(), L.scan(), r->verts.p, r->offsets.p,
                               r->indices.p, r->weights.p);
            return 0;
        });
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipStreamSynchronize(st));   // the scratch is released on return
    held_replace(c, HELD_ELEVATION, r);
    c->last_kernel = "k_label_keys + radix sort + k_label_first + scan + k_elevate_cells + k_elevate_rows";
    return FH_OK;
}

}  // namespace

extern "C" {

int fh_refine_uniform(fh_ctx* c, uint64_t* out_num_vertices, uint64_t* out_num_cells, uint64_t* out_nnz) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (c->ragged) return c->fail(FH_UNSUPPORTED, "fh_refine_uniform: ragged generic connectivity cannot be refined");
    if (!c->has_mesh) return c->fail(FH_INVALID_STATE, "fh_refine_uniform: no mesh set");
    LabelTable t;
    RefineChildren ch;
    if (!refine_table(c->elem_kind, t, ch)) return c->fail(FH_UNSUPPORTED, "fh_refine_uniform: uniform refinement covers Tet4, Tri3, Quad4 and Hex8");
    int rc = refine_uniform(c, t, ch);
    if (rc) return rc;
    const HeldMesh* r = c->held[HELD_REFINEMENT];
    if (out_num_vertices) *out_num_vertices = r->num_vertices;
    if (out_num_cells) *out_num_cells = r->num_cells;
    if (out_nnz) *out_nnz = r->nnz;
    return FH_OK;
}

int fh_refinement_mesh(fh_ctx* c, double* vertices, uint64_t* connectivity) {
    return held_mesh(c, HELD_REFINEMENT, "fh_refinement_mesh", vertices, connectivity, nullptr);
}

int fh_refinement_transfer(fh_ctx* c, uint64_t* offsets, uint64_t* indices, double* weights) {
    return held_transfer(c, HELD_REFINEMENT, "fh_refinement_transfer", offsets, indices, weights);
}

int fh_set_mesh_from_refinement(fh_ctx* fine, fh_ctx* coarse) {
    return held_hand_over(fine, coarse, HELD_REFINEMENT, "fh_set_mesh_from_refinement");
}

int fh_coarsen_degree(fh_ctx* c, uint64_t* out_num_vertices, uint64_t* out_nnz) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (c->ragged) return c->fail(FH_UNSUPPORTED, "fh_coarsen_degree: ragged generic connectivity has no degree to coarsen");
    if (!c->has_mesh) return c->fail(FH_INVALID_STATE, "fh_coarsen_degree: no mesh set");
    CoarsenTable t;
    int linear_kind = -1;
    if (!coarsen_table(c->elem_kind, t, linear_kind))
        return c->fail(FH_UNSUPPORTED, "fh_coarsen_degree: degree coarsening covers Tet10, Tri6, Quad9, Hex20 and Hex27");
    int rc = coarsen_degree(c, t, linear_kind);
    if (rc) return rc;
    if (out_num_vertices) *out_num_vertices = c->held[HELD_COARSENING]->num_vertices;
    if (out_nnz) *out_nnz = c->held[HELD_COARSENING]->nnz;
    return FH_OK;
}

int fh_degree_coarsening_mesh(fh_ctx* c, double* vertices, uint64_t* connectivity, uint64_t* vertex_nodes) {
    return held_mesh(c, HELD_COARSENING, "fh_degree_coarsening_mesh", vertices, connectivity, vertex_nodes);
}

int fh_degree_coarsening_transfer(fh_ctx* c, uint64_t* offsets, uint64_t* indices, double* weights) {
    return held_transfer(c, HELD_COARSENING, "fh_degree_coarsening_transfer", offsets, indices, weights);
}

int fh_set_mesh_from_degree_coarsening(fh_ctx* linear, fh_ctx* high) {
    return held_hand_over(linear, high, HELD_COARSENING, "fh_set_mesh_from_degree_coarsening");
}

int fh_elevate_degree(fh_ctx* c, int to_kind, uint64_t* out_num_vertices, uint64_t* out_nnz) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (c->ragged) return c->fail(FH_UNSUPPORTED, "fh_elevate_degree: ragged generic connectivity has no degree to elevate");
    if (!c->has_mesh) return c->fail(FH_INVALID_STATE, "fh_elevate_degree: no mesh set");
    const int from = c->elem_kind;
    if (from != FH_TET4 && from != FH_TRI3 && from != FH_QUAD4 && from != FH_HEX8)
        return c->fail(FH_UNSUPPORTED, "fh_elevate_degree: degree elevation starts from Tet4, Tri3, Quad4 or Hex8");
    CoarsenTable high;
    int linear_kind = -1;
    if (!coarsen_table(to_kind, high, linear_kind) || linear_kind != from)
        return c->fail(FH_BAD_ARGUMENT, "fh_elevate_degree: the conversions are Tet4 -> Tet10, Tri3 -> Tri6, Quad4 -> Quad9, Hex8 -> Hex20 and Hex8 -> Hex27");
    const int keep = (to_kind == FH_TRI6 || to_kind == FH_QUAD9) ? 1 : 0;
    const int centre = (to_kind == FH_QUAD9 || to_kind == FH_HEX27) ? 1 : 0;   // the last node of these is the cell's centre: not matched
    int rc = elevate_degree(c, label_table(high, keep ? high.nv : 0, centre, keep), to_kind);
    if (rc) return rc;
    if (out_num_vertices) *out_num_vertices = c->held[HELD_ELEVATION]->num_vertices;
    if (out_nnz) *out_nnz = c->held[HELD_ELEVATION]->nnz;
    return FH_OK;
}

int fh_degree_elevation_mesh(fh_ctx* c, double* vertices, uint64_t* connectivity) {
    return held_mesh(c, HELD_ELEVATION, "fh_degree_elevation_mesh", vertices, connectivity, nullptr);
}

int fh_degree_elevation_transfer(fh_ctx* c, uint64_t* offsets, uint64_t* indices, double* weights) {
    return held_transfer(c, HELD_ELEVATION, "fh_degree_elevation_transfer", offsets, indices, weights);
}

int fh_set_mesh_from_degree_elevation(fh_ctx* high, fh_ctx* linear) {
    return held_hand_over(high, linear, HELD_ELEVATION, "fh_set_mesh_from_degree_elevation");
}

}  // extern "C"
