// Uniform refinement of the context's mesh on the device, with the transfer from the coarse vertices to the fine ones (what
// fh_refine_hex8_uniform does on the host for Hex8; the reference's refine_uniformly, src/mesh/refinement.rs, covers Tri3).
// DESIGN.md section 3.6.3a.
#include "engine_internal.hpp"
#include "refine_kernels.hpp"

#include <memory>

namespace {

constexpr int_list<FH_TET4, FH_TRI3, FH_QUAD4, FH_HEX8> refine_kinds{};
// most parents of a new point, and the dimension
template <int EK> struct refine_geom {
    static constexpr int MP = (EK == FH_HEX8) ? 8 : (EK == FH_QUAD4) ? 4 : 2;
    static constexpr int D = kind_geom<EK>::D;
};

RefineTable simple_table(int n, int P, int C, const int (*par)[4], const int* cnt, const int (*child)[4]) {
    RefineTable t{};
    t.n = n; t.P = P; t.C = C;
    for (int p = 0; p < P; ++p) {
        t.cnt[p] = (signed char)cnt[p];
        for (int q = 0; q < cnt[p]; ++q) t.par[p][q] = (signed char)par[p][q];
    }
    for (int k = 0; k < C; ++k)
        for (int a = 0; a < n; ++a) t.child[k][a] = (signed char)child[k][a];
    return t;
}

// Tet4: the edges in the Tet10 order (fh_refine_to_quadratic); Bey's red refinement, the inner octahedron cut along (0,2)-(1,3), nodes
// 1 and 3 of the two inner children that Bey's own order leaves negatively oriented swapped.  All eight children have the parent's
// orientation and 1/8 of its volume, and repeated refinement stays within 3 congruence classes: any other choice of swaps does not.
RefineTable tet4_table() {
    static const int PAR[6][4] = {{0, 1}, {1, 2}, {0, 2}, {0, 3}, {2, 3}, {1, 3}};
    static const int CNT[6] = {2, 2, 2, 2, 2, 2};
    static const int CH[8][4] = {{0, 4, 6, 7}, {4, 1, 5, 9}, {6, 5, 2, 8}, {7, 9, 8, 3}, {4, 6, 7, 9}, {4, 9, 5, 6}, {6, 7, 9, 8}, {6, 8, 9, 5}};
    return simple_table(4, 6, 8, PAR, CNT, CH);
}
// Tri3: detail.rs:116-127 with d, e, f = 3, 4, 5
RefineTable tri3_table() {
    static const int PAR[3][4] = {{0, 1}, {1, 2}, {2, 0}};
    static const int CNT[3] = {2, 2, 2};
    static const int CH[4][4] = {{0, 3, 5}, {3, 1, 4}, {5, 4, 2}, {3, 4, 5}};
    return simple_table(3, 3, 4, PAR, CNT, CH);
}
RefineTable quad4_table() {
    static const int PAR[5][4] = {{0, 1}, {1, 2}, {2, 3}, {3, 0}, {0, 1, 2, 3}};
    static const int CNT[5] = {2, 2, 2, 2, 4};
    static const int CH[4][4] = {{0, 4, 8, 7}, {4, 1, 5, 8}, {8, 5, 2, 6}, {7, 8, 6, 3}};
    return simple_table(4, 5, 4, PAR, CNT, CH);
}
// Hex8: the 3x3x3 lattice of refine_hex8_uniform (host_inputs.cpp), x fastest; a lattice point's parents are the corners that agree
// with it on its nonzero axes, in ascending local node; child (cx, cy, cz) takes the lattice points (cx, cy, cz) + its nodes' offsets
RefineTable hex8_table() {
    RefineTable t{};
    t.n = 8; t.C = 8;
    int lat[27], P = 0;
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
                t.cnt[P] = (signed char)cnt;
                for (int q = 0; q < cnt; ++q) t.par[P][q] = (signed char)par[q];
                lat[i + 3 * j + 9 * k] = 8 + P++;
            }
    t.P = P;
    for (int cz = 0; cz < 2; ++cz)
        for (int cy = 0; cy < 2; ++cy)
            for (int cx = 0; cx < 2; ++cx)
                for (int a = 0; a < 8; ++a) {
                    const int i = cx + ((int)HEX_SIGN[a][0] + 1) / 2, j = cy + ((int)HEX_SIGN[a][1] + 1) / 2, k = cz + ((int)HEX_SIGN[a][2] + 1) / 2;
                    t.child[cx + 2 * cy + 4 * cz][a] = (signed char)lat[i + 3 * j + 9 * k];
                }
    return t;
}

bool refine_table(int kind, RefineTable& t) {
    switch (kind) {
        case FH_TET4: t = tet4_table(); return true;
        case FH_TRI3: t = tri3_table(); return true;
        case FH_QUAD4: t = quad4_table(); return true;
        case FH_HEX8: t = hex8_table(); return true;
        default: return false;
    }
}

}  // namespace

// the held refinement: the fine mesh and the transfer (CSR by fine vertex), on the device
struct RefineStore {
    int elem_kind = -1, d = 0, n = 0;
    uint64_t num_vertices = 0, num_cells = 0, nnz = 0, num_coarse = 0;
    DevBuf<double> verts, weights;
    DevBuf<unsigned long long> conn, offsets, indices;
    uint64_t scratch_bytes = 0;
};

extern "C++" void refine_drop(fh_ctx* c) {
    delete c->refined;
    c->refined = nullptr;
}

static int refine_uniform(fh_ctx* c, const RefineTable& t) {
    hipStream_t st = c->stream;
    const unsigned N = (unsigned)c->N;
    const uint64_t nocc64 = c->E * (uint64_t)t.P;
    if (nocc64 >= (1ull << 31)) return c->fail(FH_UNSUPPORTED, "fh_refine_uniform: num_elements * new points per cell must be < 2^31");
    const unsigned nocc = (unsigned)nocc64;
    int bits = 1;
    while ((1ull << bits) < c->N) ++bits;
    auto r = std::make_unique<RefineStore>();
    r->elem_kind = c->elem_kind;
    r->d = c->ei.d;
    r->n = t.n;
    r->num_coarse = c->N;
    r->num_cells = c->E * (uint64_t)t.C;
    // scratch, 24 bytes per occurrence: keys and ids, twice each for the sort.  Once sorted, the unsorted keys hold the scan's input, the
    // unsorted ids the first occurrences; after stage 3 the sorted keys hold the scan, the sorted ids the fine indices.
    DevBuf<unsigned long long> keys_in, keys;
    DevBuf<unsigned> ids_in, ids;
    DevBuf<char> tmp;
    uint64_t M = 0, new_nnz = 0;
    const int grid = (int)((nocc + 255u) / 256u);
    if (nocc) {
        HIP_TRY(c, keys_in.alloc(nocc));
        HIP_TRY(c, keys.alloc(nocc));
        HIP_TRY(c, ids_in.alloc(nocc));
        HIP_TRY(c, ids.alloc(nocc));
        size_t sort_bytes = 0, scan_bytes = 0;
        HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, keys_in.p, keys.p, ids_in.p, ids.p, (int)nocc, 0, 2 * bits, st));
        HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, keys_in.p, keys.p, (int)nocc, st));
        HIP_TRY(c, tmp.alloc(std::max(sort_bytes, scan_bytes)));
        r->scratch_bytes = (uint64_t)nocc * 24 + std::max(sort_bytes, scan_bytes);
        dispatch(refine_kinds, c->elem_kind, 0, [&](auto ek) {
            hipLaunchKernelGGL(k_refine_keys<refine_geom<ek()>::MP>, dim3(grid), dim3(256), 0, st, c->conn.p, t, nocc, bits, keys_in.p, ids_in.p);
            return 0;
        });
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(tmp.p, sort_bytes, keys_in.p, keys.p, ids_in.p, ids.p, (int)nocc, 0, 2 * bits, st));
        unsigned* first = ids_in.p;
        unsigned long long* val = keys_in.p;
        dispatch(refine_kinds, c->elem_kind, 0, [&](auto ek) {
            hipLaunchKernelGGL(k_refine_first<refine_geom<ek()>::MP>, dim3(grid), dim3(256), 0, st, c->conn.p, t, nocc, keys.p, ids.p, first, val);
            return 0;
        });
        HIP_TRY(c, hipGetLastError());
        unsigned long long* scan = keys.p;
        HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(tmp.p, scan_bytes, val, scan, (int)nocc, st));
        unsigned long long tail[2] = {0, 0};
        HIP_TRY(c, hipMemcpyAsync(&tail[0], val + (nocc - 1), sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(&tail[1], scan + (nocc - 1), sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        const unsigned long long total = tail[0] + tail[1];
        M = total >> 33;
        new_nnz = total & ((1ull << 33) - 1);
    }
    r->num_vertices = c->N + M;
    r->nnz = c->N + new_nnz;
    if (r->num_vertices >= (1ull << 31)) return c->fail(FH_UNSUPPORTED, "fh_refine_uniform: the refined mesh must have < 2^31 vertices");
    HIP_TRY(c, r->verts.alloc((size_t)r->num_vertices * r->d));
    HIP_TRY(c, r->conn.alloc((size_t)r->num_cells * t.n));
    HIP_TRY(c, r->offsets.alloc((size_t)r->num_vertices + 1));
    HIP_TRY(c, r->indices.alloc((size_t)r->nnz));
    HIP_TRY(c, r->weights.alloc((size_t)r->nnz));
    dispatch_or_last(int_list<2, 3>{}, r->d, [&](auto d) {
        hipLaunchKernelGGL(k_refine_coarse_rows<d()>, dim3(N / 256u + 1u), dim3(256), 0, st, c->verts.p, N, (unsigned long long)r->num_vertices,
                           (unsigned long long)r->nnz, r->verts.p, r->offsets.p, r->indices.p, r->weights.p);
        return 0;
    });
    HIP_TRY(c, hipGetLastError());
    if (nocc) {
        unsigned* first = ids_in.p;
        unsigned* fine = ids.p;
        const unsigned long long* scan = keys.p;
        hipLaunchKernelGGL(k_refine_fine_index, dim3(grid), dim3(256), 0, st, nocc, N, first, scan, fine);
        HIP_TRY(c, hipGetLastError());
        const unsigned long long total = (unsigned long long)r->num_cells * t.n;
        hipLaunchKernelGGL(k_refine_children, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, c->conn.p, t, total, fine, r->conn.p);
        HIP_TRY(c, hipGetLastError());
        dispatch(refine_kinds, c->elem_kind, 0, [&](auto ek) {
            hipLaunchKernelGGL((k_refine_new_rows<refine_geom<ek()>::MP, refine_geom<ek()>::D>), dim3(grid), dim3(256), 0, st, c->verts.p, c->conn.p, t,
                               nocc, N, first, scan, r->verts.p, r->offsets.p, r->indices.p, r->weights.p);
            return 0;
        });
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipStreamSynchronize(st));   // the scratch is released on return
    refine_drop(c);
    c->refined = r.release();
    c->last_kernel = "k_refine_keys + radix sort + k_refine_first + scan + k_refine_fine_index + k_refine_children + k_refine_new_rows";
    return FH_OK;
}

static int held(fh_ctx* c, const char* who) {
    if (!c->refined) return c->fail(FH_INVALID_STATE, std::string(who) + ": no refinement held (fh_refine_uniform; fh_set_mesh* drops it)");
    return FH_OK;
}

extern "C" {

int fh_refine_uniform(fh_ctx* c, uint64_t* out_num_vertices, uint64_t* out_num_cells, uint64_t* out_nnz) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (c->ragged) return c->fail(FH_UNSUPPORTED, "fh_refine_uniform: ragged generic connectivity cannot be refined");
    if (!c->has_mesh) return c->fail(FH_INVALID_STATE, "fh_refine_uniform: no mesh set");
    RefineTable t;
    if (!refine_table(c->elem_kind, t)) return c->fail(FH_UNSUPPORTED, "fh_refine_uniform: uniform refinement covers Tet4, Tri3, Quad4 and Hex8");
    int rc = refine_uniform(c, t);
    if (rc) return rc;
    if (out_num_vertices) *out_num_vertices = c->refined->num_vertices;
    if (out_num_cells) *out_num_cells = c->refined->num_cells;
    if (out_nnz) *out_nnz = c->refined->nnz;
    return FH_OK;
}

int fh_refinement_mesh(fh_ctx* c, double* vertices, uint64_t* connectivity) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int rc = held(c, "fh_refinement_mesh");
    if (rc) return rc;
    const RefineStore* r = c->refined;
    if (vertices && r->num_vertices)
        HIP_TRY(c, hipMemcpyAsync(vertices, r->verts.p, sizeof(double) * r->num_vertices * r->d, hipMemcpyDeviceToHost, c->stream));
    if (connectivity && r->num_cells)
        HIP_TRY(c, hipMemcpyAsync(connectivity, r->conn.p, sizeof(uint64_t) * r->num_cells * r->n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FH_OK;
}

int fh_refinement_transfer(fh_ctx* c, uint64_t* offsets, uint64_t* indices, double* weights) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int rc = held(c, "fh_refinement_transfer");
    if (rc) return rc;
    const RefineStore* r = c->refined;
    if (offsets) HIP_TRY(c, hipMemcpyAsync(offsets, r->offsets.p, sizeof(uint64_t) * (r->num_vertices + 1), hipMemcpyDeviceToHost, c->stream));
    if (indices && r->nnz) HIP_TRY(c, hipMemcpyAsync(indices, r->indices.p, sizeof(uint64_t) * r->nnz, hipMemcpyDeviceToHost, c->stream));
    if (weights && r->nnz) HIP_TRY(c, hipMemcpyAsync(weights, r->weights.p, sizeof(double) * r->nnz, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FH_OK;
}

int fh_set_mesh_from_refinement(fh_ctx* fine, fh_ctx* coarse) {
    if (!fine || !coarse) return FH_BAD_ARGUMENT;
    if (held(coarse, "fh_set_mesh_from_refinement")) return fine->fail(FH_INVALID_STATE, coarse->err);
    if (fine->device != coarse->device) return fine->fail(FH_BAD_ARGUMENT, "fh_set_mesh_from_refinement: the two contexts are on different devices");
    // fh_set_mesh_dev drops the refinement its context holds: taken off the coarse context for the call, so that fine == coarse works
    RefineStore* r = coarse->refined;
    coarse->refined = nullptr;
    {
        DevGuard dev_guard_(coarse->device);
        (void)hipStreamSynchronize(coarse->stream);   // (the result was formed on the coarse context's stream)
    }
    const int rc = fh_set_mesh_dev(fine, r->elem_kind, r->verts.p, r->num_vertices, reinterpret_cast<const uint64_t*>(r->conn.p), r->num_cells);
    if (fine == coarse) delete r;
    else coarse->refined = r;
    return rc;
}

}  // extern "C"
