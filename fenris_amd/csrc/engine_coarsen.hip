// Degree coarsening of the context's mesh on the device: the linear mesh on the vertex nodes of a Tet10, Tri6, Quad9, Hex20 or Hex27
// mesh and the transfer that interpolates linear nodal values to all of its nodes (the p-coarsening step of a multigrid hierarchy).
// DESIGN.md section 3.6.3b.
#include "engine_internal.hpp"
#include "coarsen_kernels.hpp"

#include <memory>

namespace {

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

constexpr int_list<2, 4, 8> coarsen_parents{};

}  // namespace

// the held degree coarsening: the linear mesh, the fine indices of its vertices and the transfer (CSR by fine node), on the device
struct CoarsenStore {
    int elem_kind = -1, d = 0, nv = 0;
    uint64_t num_vertices = 0, num_cells = 0, num_fine = 0, nnz = 0;
    DevBuf<double> verts, weights;
    DevBuf<unsigned long long> conn, vertex_nodes, offsets, indices;
};

extern "C++" void coarsen_drop(fh_ctx* c) {
    delete c->coarsened;
    c->coarsened = nullptr;
}

static int coarsen_degree(fh_ctx* c, const CoarsenTable& t, int linear_kind) {
    hipStream_t st = c->stream;
    const unsigned N = (unsigned)c->N;
    int mp = 1;
    for (int l = 0; l < t.n; ++l) mp = std::max(mp, (int)t.cnt[l]);
    const uint64_t nocc64 = c->E * (uint64_t)t.n;
    if (nocc64 >= (1ull << 31)) return c->fail(FH_UNSUPPORTED, "fh_coarsen_degree: num_elements * nodes per cell must be < 2^31");
    if (c->N * (uint64_t)mp >= (1ull << 31))
        return c->fail(FH_UNSUPPORTED, "fh_coarsen_degree: num_vertices * most parents of a node must be < 2^31");
    const unsigned nocc = (unsigned)nocc64;
    auto r = std::make_unique<CoarsenStore>();
    r->elem_kind = linear_kind;
    r->d = c->ei.d;
    r->nv = t.nv;
    r->num_cells = c->E;
    r->num_fine = c->N;
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
            dispatch(coarsen_parents, mp, 0, [&](auto m) {
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
    HIP_TRY(c, r->verts.alloc((size_t)M * r->d));
    HIP_TRY(c, r->vertex_nodes.alloc(M));
    HIP_TRY(c, r->conn.alloc((size_t)r->num_cells * t.nv));
    HIP_TRY(c, r->offsets.alloc((size_t)N + 1));
    HIP_TRY(c, r->indices.alloc((size_t)r->nnz));
    HIP_TRY(c, r->weights.alloc((size_t)r->nnz));
    dispatch(coarsen_parents, mp, 0, [&](auto m) {
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
    coarsen_drop(c);
    c->coarsened = r.release();
    c->last_kernel = "k_coarsen_owner + k_coarsen_flags + k_coarsen_check + scan + k_coarsen_rows + k_coarsen_cells + k_coarsen_vertices";
    return FH_OK;
}

static int held(fh_ctx* c, const char* who) {
    if (!c->coarsened) return c->fail(FH_INVALID_STATE, std::string(who) + ": no degree coarsening held (fh_coarsen_degree; fh_set_mesh* drops it)");
    return FH_OK;
}

extern "C" {

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
    if (out_num_vertices) *out_num_vertices = c->coarsened->num_vertices;
    if (out_nnz) *out_nnz = c->coarsened->nnz;
    return FH_OK;
}

int fh_degree_coarsening_mesh(fh_ctx* c, double* vertices, uint64_t* connectivity, uint64_t* vertex_nodes) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int rc = held(c, "fh_degree_coarsening_mesh");
    if (rc) return rc;
    const CoarsenStore* r = c->coarsened;
    if (vertices && r->num_vertices)
        HIP_TRY(c, hipMemcpyAsync(vertices, r->verts.p, sizeof(double) * r->num_vertices * r->d, hipMemcpyDeviceToHost, c->stream));
    if (connectivity && r->num_cells)
        HIP_TRY(c, hipMemcpyAsync(connectivity, r->conn.p, sizeof(uint64_t) * r->num_cells * r->nv, hipMemcpyDeviceToHost, c->stream));
    if (vertex_nodes && r->num_vertices)
        HIP_TRY(c, hipMemcpyAsync(vertex_nodes, r->vertex_nodes.p, sizeof(uint64_t) * r->num_vertices, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FH_OK;
}

int fh_degree_coarsening_transfer(fh_ctx* c, uint64_t* offsets, uint64_t* indices, double* weights) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int rc = held(c, "fh_degree_coarsening_transfer");
    if (rc) return rc;
    const CoarsenStore* r = c->coarsened;
    if (offsets) HIP_TRY(c, hipMemcpyAsync(offsets, r->offsets.p, sizeof(uint64_t) * (r->num_fine + 1), hipMemcpyDeviceToHost, c->stream));
    if (indices && r->nnz) HIP_TRY(c, hipMemcpyAsync(indices, r->indices.p, sizeof(uint64_t) * r->nnz, hipMemcpyDeviceToHost, c->stream));
    if (weights && r->nnz) HIP_TRY(c, hipMemcpyAsync(weights, r->weights.p, sizeof(double) * r->nnz, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FH_OK;
}

int fh_set_mesh_from_degree_coarsening(fh_ctx* linear, fh_ctx* high) {
    if (!linear || !high) return FH_BAD_ARGUMENT;
    if (held(high, "fh_set_mesh_from_degree_coarsening")) return linear->fail(FH_INVALID_STATE, high->err);
    if (linear->device != high->device)
        return linear->fail(FH_BAD_ARGUMENT, "fh_set_mesh_from_degree_coarsening: the two contexts are on different devices");
    // fh_set_mesh_dev drops the coarsening its context holds: taken off the high context for the call, so that linear == high works
    CoarsenStore* r = high->coarsened;
    high->coarsened = nullptr;
    {
        DevGuard dev_guard_(high->device);
        (void)hipStreamSynchronize(high->stream);   // (the result was formed on the high context's stream)
    }
    const int rc = fh_set_mesh_dev(linear, r->elem_kind, r->verts.p, r->num_vertices, reinterpret_cast<const uint64_t*>(r->conn.p), r->num_cells);
    if (linear == high) delete r;
    else high->coarsened = r;
    return rc;
}

}  // extern "C"
