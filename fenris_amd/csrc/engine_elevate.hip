// Degree elevation of the context's mesh on the device: the Tet10, Tri6, Quad9, Hex20 or Hex27 mesh over a linear one, numbered and placed
// bit for bit as fh_refine_to_quadratic and fh_hex8_to_hex27 do on the host (host_inputs.cpp), and the transfer that interpolates linear
// nodal values to all of its nodes (the p-step of a multigrid hierarchy, formed with the mesh).  DESIGN.md section 3.6.3c.
#include "engine_internal.hpp"
#include "elevate_kernels.hpp"

#include <memory>

namespace {

constexpr int_list<2, 4> elevate_matched_parents{};
constexpr int_list<2, 4, 8> elevate_parents{};

}  // namespace

// the held degree elevation: the high mesh and the transfer (CSR by high node over the linear vertices), on the device
struct ElevateStore {
    int elem_kind = -1, d = 0, n = 0;
    uint64_t num_vertices = 0, num_cells = 0, nnz = 0, num_linear = 0;
    DevBuf<double> verts, weights;
    DevBuf<unsigned long long> conn, offsets, indices;
    uint64_t scratch_bytes = 0;
};

extern "C++" void elevate_drop(fh_ctx* c) {
    delete c->elevated;
    c->elevated = nullptr;
}

static int elevate_degree(fh_ctx* c, const ElevateTable& t, int to_kind) {
    hipStream_t st = c->stream;
    const unsigned N = (unsigned)c->N;
    const int n = t.t.n;
    if (c->E * (uint64_t)n >= (1ull << 31)) return c->fail(FH_UNSUPPORTED, "fh_elevate_degree: num_elements * nodes per high cell must be < 2^31");
    const unsigned E = (unsigned)c->E;
    const unsigned nlab = E * (unsigned)t.S, nsort = E * (unsigned)t.Sm;
    const unsigned base = t.keep ? N : 0u;
    int mp_matched = 1, mp = 1;
    for (int l = t.s0; l < n; ++l) {
        mp = std::max(mp, (int)t.t.cnt[l]);
        if (l < t.s0 + t.Sm) mp_matched = std::max(mp_matched, (int)t.t.cnt[l]);
    }
    int bits = 1;
    while ((1ull << bits) <= c->N) ++bits;   // N itself is the second parent of a vertex candidate
    auto r = std::make_unique<ElevateStore>();
    r->elem_kind = to_kind;
    r->d = c->ei.d;
    r->n = n;
    r->num_linear = c->N;
    r->num_cells = c->E;
    // scratch, 24 bytes per candidate: keys and ids, twice each for the sort.  Once sorted, the unsorted keys hold the scan's input, the
    // unsorted ids the first candidates; after stage 3 the sorted keys hold the scan.
    DevBuf<unsigned long long> keys_in, keys;
    DevBuf<unsigned> ids_in, ids;
    DevBuf<char> tmp;
    uint64_t M = 0, lab_nnz = 0;
    const int sort_grid = (int)((nsort + 255u) / 256u), lab_grid = (int)((nlab + 255u) / 256u);
    if (nlab) {
        HIP_TRY(c, keys_in.alloc(nlab));
        HIP_TRY(c, keys.alloc(nlab));
        HIP_TRY(c, ids_in.alloc(nlab));
        HIP_TRY(c, ids.alloc(nlab));
        size_t sort_bytes = 0, scan_bytes = 0;
        HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, keys_in.p, keys.p, ids_in.p, ids.p, (int)nsort, 0, 2 * bits, st));
        HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, keys_in.p, keys.p, (int)nlab, st));
        HIP_TRY(c, tmp.alloc(std::max(sort_bytes, scan_bytes)));
        r->scratch_bytes = (uint64_t)nlab * 24 + std::max(sort_bytes, scan_bytes);
        dispatch(elevate_matched_parents, std::max(mp_matched, 2), 0, [&](auto m) {
            hipLaunchKernelGGL(k_elevate_keys<m()>, dim3(sort_grid), dim3(256), 0, st, c->conn.p, t, nsort, N, bits, keys_in.p, ids_in.p);
            return 0;
        });
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(tmp.p, sort_bytes, keys_in.p, keys.p, ids_in.p, ids.p, (int)nsort, 0, 2 * bits, st));
        unsigned* first = ids_in.p;
        unsigned long long* val = keys_in.p;
        dispatch(elevate_matched_parents, std::max(mp_matched, 2), 0, [&](auto m) {
            hipLaunchKernelGGL(k_elevate_first<m()>, dim3(sort_grid), dim3(256), 0, st, c->conn.p, t, nsort, E, keys.p, ids.p, first, val);
            return 0;
        });
        HIP_TRY(c, hipGetLastError());
        unsigned long long* scan = keys.p;
        HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(tmp.p, scan_bytes, val, scan, (int)nlab, st));
        unsigned long long tail[2] = {0, 0};
        HIP_TRY(c, hipMemcpyAsync(&tail[0], val + (nlab - 1), sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipMemcpyAsync(&tail[1], scan + (nlab - 1), sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(c, hipStreamSynchronize(st));
        const unsigned long long total = tail[0] + tail[1];
        M = total >> ELEVATE_SHIFT;
        lab_nnz = total & ((1ull << ELEVATE_SHIFT) - 1);
    }
    r->num_vertices = base + M;
    r->nnz = base + lab_nnz;
    if (r->num_vertices >= (1ull << 31)) return c->fail(FH_UNSUPPORTED, "fh_elevate_degree: the high mesh must have < 2^31 nodes");
    HIP_TRY(c, r->verts.alloc((size_t)r->num_vertices * r->d));
    HIP_TRY(c, r->conn.alloc((size_t)r->num_cells * n));
    HIP_TRY(c, r->offsets.alloc((size_t)r->num_vertices + 1));
    HIP_TRY(c, r->indices.alloc((size_t)r->nnz));
    HIP_TRY(c, r->weights.alloc((size_t)r->nnz));
    if (t.keep) {
        // the kept vertices: their positions and identity rows; thread N closes the offsets
        dispatch_or_last(int_list<2, 3>{}, r->d, [&](auto d) {
            hipLaunchKernelGGL(k_refine_coarse_rows<d()>, dim3(N / 256u + 1u), dim3(256), 0, st, c->verts.p, N, (unsigned long long)r->num_vertices,
                               (unsigned long long)r->nnz, r->verts.p, r->offsets.p, r->indices.p, r->weights.p);
            return 0;
        });
        HIP_TRY(c, hipGetLastError());
    } else if (!nlab) {
        HIP_TRY(c, hipMemsetAsync(r->offsets.p, 0, sizeof(unsigned long long), st));
    }
    if (nlab) {
        const unsigned* first = ids_in.p;
        const unsigned long long* scan = keys.p;
        const unsigned long long total = (unsigned long long)r->num_cells * n;
        hipLaunchKernelGGL(k_elevate_cells, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, c->conn.p, t, total, base, first, scan, r->conn.p);
        HIP_TRY(c, hipGetLastError());
        dispatch(elevate_parents, std::max(mp, 2), int_list<2, 3>{}, r->d, 0, [&](auto m, auto d) {
            hipLaunchKernelGGL((k_elevate_rows<m(), d()>), dim3(lab_grid), dim3(256), 0, st, c->verts.p, c->conn.p, t, nlab, base,
                               (unsigned long long)r->num_vertices, (unsigned long long)r->nnz, first, scan, r->verts.p, r->offsets.p, r->indices.p,
                               r->weights.p);
            return 0;
        });
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipStreamSynchronize(st));   // the scratch is released on return
    elevate_drop(c);
    c->elevated = r.release();
    c->last_kernel = "k_elevate_keys + radix sort + k_elevate_first + scan + k_elevate_cells + k_elevate_rows";
    return FH_OK;
}

static int held(fh_ctx* c, const char* who) {
    if (!c->elevated) return c->fail(FH_INVALID_STATE, std::string(who) + ": no degree elevation held (fh_elevate_degree; fh_set_mesh* drops it)");
    return FH_OK;
}

extern "C" {

int fh_elevate_degree(fh_ctx* c, int to_kind, uint64_t* out_num_vertices, uint64_t* out_nnz) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (c->ragged) return c->fail(FH_UNSUPPORTED, "fh_elevate_degree: ragged generic connectivity has no degree to elevate");
    if (!c->has_mesh) return c->fail(FH_INVALID_STATE, "fh_elevate_degree: no mesh set");
    const int from = c->elem_kind;
    if (from != FH_TET4 && from != FH_TRI3 && from != FH_QUAD4 && from != FH_HEX8)
        return c->fail(FH_UNSUPPORTED, "fh_elevate_degree: degree elevation starts from Tet4, Tri3, Quad4 or Hex8");
    ElevateTable t{};
    int linear_kind = -1;
    if (!coarsen_table(to_kind, t.t, linear_kind) || linear_kind != from)
        return c->fail(FH_BAD_ARGUMENT, "fh_elevate_degree: the conversions are Tet4 -> Tet10, Tri3 -> Tri6, Quad4 -> Quad9, Hex8 -> Hex20 and Hex8 -> Hex27");
    t.keep = (to_kind == FH_TRI6 || to_kind == FH_QUAD9) ? 1 : 0;
    t.s0 = t.keep ? t.t.nv : 0;
    t.S = t.t.n - t.s0;
    t.Sm = t.S - ((to_kind == FH_QUAD9 || to_kind == FH_HEX27) ? 1 : 0);   // the last node of these is the cell's centre
    int rc = elevate_degree(c, t, to_kind);
    if (rc) return rc;
    if (out_num_vertices) *out_num_vertices = c->elevated->num_vertices;
    if (out_nnz) *out_nnz = c->elevated->nnz;
    return FH_OK;
}

int fh_degree_elevation_mesh(fh_ctx* c, double* vertices, uint64_t* connectivity) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int rc = held(c, "fh_degree_elevation_mesh");
    if (rc) return rc;
    const ElevateStore* r = c->elevated;
    if (vertices && r->num_vertices)
        HIP_TRY(c, hipMemcpyAsync(vertices, r->verts.p, sizeof(double) * r->num_vertices * r->d, hipMemcpyDeviceToHost, c->stream));
    if (connectivity && r->num_cells)
        HIP_TRY(c, hipMemcpyAsync(connectivity, r->conn.p, sizeof(uint64_t) * r->num_cells * r->n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FH_OK;
}

int fh_degree_elevation_transfer(fh_ctx* c, uint64_t* offsets, uint64_t* indices, double* weights) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int rc = held(c, "fh_degree_elevation_transfer");
    if (rc) return rc;
    const ElevateStore* r = c->elevated;
    if (offsets) HIP_TRY(c, hipMemcpyAsync(offsets, r->offsets.p, sizeof(uint64_t) * (r->num_vertices + 1), hipMemcpyDeviceToHost, c->stream));
    if (indices && r->nnz) HIP_TRY(c, hipMemcpyAsync(indices, r->indices.p, sizeof(uint64_t) * r->nnz, hipMemcpyDeviceToHost, c->stream));
    if (weights && r->nnz) HIP_TRY(c, hipMemcpyAsync(weights, r->weights.p, sizeof(double) * r->nnz, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FH_OK;
}

int fh_set_mesh_from_degree_elevation(fh_ctx* high, fh_ctx* linear) {
    if (!high || !linear) return FH_BAD_ARGUMENT;
    if (held(linear, "fh_set_mesh_from_degree_elevation")) return high->fail(FH_INVALID_STATE, linear->err);
    if (high->device != linear->device)
        return high->fail(FH_BAD_ARGUMENT, "fh_set_mesh_from_degree_elevation: the two contexts are on different devices");
    // fh_set_mesh_dev drops the elevation its context holds: taken off the linear context for the call, so that high == linear works
    ElevateStore* r = linear->elevated;
    linear->elevated = nullptr;
    {
        DevGuard dev_guard_(linear->device);
        (void)hipStreamSynchronize(linear->stream);   // (the result was formed on the linear context's stream)
    }
    const int rc = fh_set_mesh_dev(high, r->elem_kind, r->verts.p, r->num_vertices, reinterpret_cast<const uint64_t*>(r->conn.p), r->num_cells);
    if (high == linear) delete r;
    else linear->elevated = r;
    return rc;
}

}  // extern "C"
