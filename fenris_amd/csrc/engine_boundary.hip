// Boundary faces of the context's mesh (Mesh::find_boundary_faces / _vertices / _cells, src/mesh.rs:154-216) and the surface load
// vector on a list of (cell, local face) pairs.  DESIGN.md section 3.7.
#include "engine_internal.hpp"
#include "boundary_kernels.hpp"

// ---- face tables: get_face_connectivity of every cell kind, restated (src/connectivity.rs) -----------------------------------------
namespace {
const FaceTable FT_NONE = {0, 0, {{0}}};   // Tet20: num_faces() == 0 (connectivity.rs:977-987)
const FaceTable FT_QUAD4 = {4, 2, {{0, 1}, {1, 2}, {2, 3}, {3, 0}}};                       // :205-212  [i, (i + 1) % 4]
const FaceTable FT_TRI3 = {3, 2, {{0, 1}, {1, 2}, {2, 0}}};                                // :252-259  [i, (i + 1) % 3]
const FaceTable FT_TRI6 = {3, 3, {{0, 3, 1}, {1, 4, 2}, {2, 5, 0}}};                       // :340-351  [i, i + 3, (i + 1) % 3]
const FaceTable FT_QUAD9 = {4, 3, {{0, 4, 1}, {1, 5, 2}, {2, 6, 3}, {3, 7, 0}}};           // :414-423
const FaceTable FT_TET4 = {4, 3, {{0, 2, 1}, {0, 1, 3}, {1, 2, 3}, {0, 3, 2}}};            // :532-543
const FaceTable FT_HEX8 = {6, 4, {{3, 2, 1, 0}, {0, 1, 5, 4}, {1, 2, 6, 5}, {2, 3, 7, 6}, {4, 7, 3, 0}, {5, 6, 7, 4}}};   // :616-634
const FaceTable FT_HEX27 = {6, 9, {{0, 3, 2, 1, 9, 13, 11, 8, 20}, {0, 1, 5, 4, 8, 12, 16, 10, 21}, {1, 2, 6, 5, 11, 14, 18, 12, 23},
                                   {2, 3, 7, 6, 13, 15, 19, 14, 24}, {0, 4, 7, 3, 10, 17, 15, 9, 22}, {4, 5, 6, 7, 16, 18, 19, 17, 25}}};   // :687-695
const FaceTable FT_HEX20 = {6, 8, {{0, 3, 2, 1, 9, 13, 11, 8}, {0, 1, 5, 4, 8, 12, 16, 10}, {1, 2, 6, 5, 11, 14, 18, 12},
                                   {2, 3, 7, 6, 13, 15, 19, 14}, {0, 4, 7, 3, 10, 17, 15, 9}, {4, 5, 6, 7, 16, 18, 19, 17}}};   // :753-760
const FaceTable FT_TET10 = {4, 6, {{0, 2, 1, 6, 5, 4}, {0, 1, 3, 4, 9, 7}, {1, 2, 3, 5, 8, 9}, {0, 3, 2, 7, 8, 6}}};   // :930-936

const FaceTable& face_table(int kind) {
    switch (kind) {
        case FH_QUAD4: return FT_QUAD4;
        case FH_TRI3: return FT_TRI3;
        case FH_TRI6: return FT_TRI6;
        case FH_QUAD9: return FT_QUAD9;
        case FH_TET4: return FT_TET4;
        case FH_HEX8: return FT_HEX8;
        case FH_HEX27: return FT_HEX27;
        case FH_HEX20: return FT_HEX20;
        case FH_TET10: return FT_TET10;
        default: return FT_NONE;
    }
}

// reference coordinates of the corners of the simplices (the hexahedra and quadrilaterals: HEX_SIGN / QUAD_SIGN)
const double TET_REF[4][3] = {{-1, -1, -1}, {1, -1, -1}, {-1, 1, -1}, {-1, -1, 1}};
const double TRI_REF[3][2] = {{-1, -1}, {1, -1}, {-1, 1}};
void corner_ref(int geom_kind, int node, double* xi) {
    switch (geom_kind) {
        case FH_HEX8: for (int k = 0; k < 3; ++k) xi[k] = HEX_SIGN[node][k]; break;
        case FH_TET4: for (int k = 0; k < 3; ++k) xi[k] = TET_REF[node][k]; break;
        case FH_QUAD4: for (int k = 0; k < 2; ++k) xi[k] = QUAD_SIGN[node][k]; break;
        default: for (int k = 0; k < 2; ++k) xi[k] = TRI_REF[node][k]; break;
    }
}
}  // namespace

struct BoundaryStore {
    // the search
    bool has_faces = false;
    uint64_t num_faces = 0;
    int nfn = 0;
    DevBuf<unsigned long long> face_nodes, cells;
    DevBuf<unsigned> local_faces;
    bool has_verts = false, has_cells = false;
    uint64_t num_verts = 0, num_cells = 0;
    DevBuf<unsigned long long> bverts, bcells;
    uint64_t scratch_bytes = 0;   // peak scratch of the last search
    // the adjacency of the last surface-load face list: entries (node, position * nfn + face node) sorted by node, keyed on the list
    bool has_adj = false;
    uint64_t adj_faces = 0, adj_hash = 0, adj_entries = 0;
    DevBuf<unsigned> ent_node, ent;
    DevBuf<unsigned long long> hash_tmp, hash_out;
    DevBuf<char> hash_cub;
    // the face-point records of the last face rule
    std::vector<double> rule_w, rule_pts;
    DevBuf<FacePointRec> recs;
    DevBuf<double> w;
    bool has_recs = false;
};

extern "C++" void boundary_drop(fh_ctx* c) {
    delete c->bnd;
    c->bnd = nullptr;
}

static BoundaryStore* store(fh_ctx* c) {
    if (!c->bnd) c->bnd = new BoundaryStore();
    return c->bnd;
}

static int boundary_ready(fh_ctx* c, const char* who) {
    if (c->ragged) return c->fail(FH_UNSUPPORTED, std::string(who) + ": ragged generic connectivity has no faces");
    if (!c->has_mesh) return c->fail(FH_INVALID_STATE, std::string(who) + ": no mesh set");
    return FH_OK;
}

// nodes per face of the ten element kinds (any other count: nothing is launched)
constexpr int_list<2, 3, 4, 6, 8, 9> face_node_counts{};

static int find_boundary_faces(fh_ctx* c) {
    BoundaryStore* b = store(c);
    if (b->has_faces) return FH_OK;
    const FaceTable& t = face_table(c->elem_kind);
    hipStream_t st = c->stream;
    b->nfn = t.nfn;
    b->num_faces = 0;
    b->scratch_bytes = 0;
    const uint64_t nf_all64 = c->E * (uint64_t)t.nfaces;
    if (nf_all64 == 0) { b->has_faces = true; return FH_OK; }
    if (nf_all64 >= (1ull << 31)) return c->fail(FH_UNSUPPORTED, "fh_find_boundary_faces: num_elements * faces per cell must be < 2^31");
    const unsigned nf_all = (unsigned)nf_all64;
    int bits = 1;
    while ((1ull << bits) < c->N) ++bits;
    // scratch: keys twice, face ids twice; the first key buffer holds the flags and their scan once the sort is done
    DevBuf<unsigned long long> keys_in, keys;
    DevBuf<unsigned> vals_in, vals;
    DevBuf<char> tmp;
    HIP_TRY(c, keys_in.alloc(nf_all));
    HIP_TRY(c, keys.alloc(nf_all));
    HIP_TRY(c, vals_in.alloc(nf_all));
    HIP_TRY(c, vals.alloc(nf_all));
    size_t sort_bytes = 0, scan_bytes = 0;
    HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, keys_in.p, keys.p, vals_in.p, vals.p, (int)nf_all, 0, 2 * bits, st));
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (unsigned*)nullptr, (unsigned*)nullptr, (int)nf_all, st));
    HIP_TRY(c, tmp.alloc(std::max(sort_bytes, scan_bytes)));
    b->scratch_bytes = (uint64_t)nf_all * 24 + std::max(sort_bytes, scan_bytes);
    const int grid = (int)((nf_all + 255u) / 256u);
    const int n = c->ei.n;
    dispatch(face_node_counts, t.nfn, 0, [&](auto nfn) {
        hipLaunchKernelGGL(k_face_keys<nfn()>, dim3(grid), dim3(256), 0, st, c->conn.p, n, t, nf_all, bits, keys_in.p, vals_in.p);
        return 0;
    });
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(tmp.p, sort_bytes, keys_in.p, keys.p, vals_in.p, vals.p, (int)nf_all, 0, 2 * bits, st));
    unsigned* flag = reinterpret_cast<unsigned*>(keys_in.p);
    unsigned* scan = flag + nf_all;
    dispatch(face_node_counts, t.nfn, 0, [&](auto nfn) {
        hipLaunchKernelGGL(k_face_unique<nfn()>, dim3(grid), dim3(256), 0, st, c->conn.p, n, t, nf_all, keys.p, vals.p, flag);
        return 0;
    });
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(tmp.p, scan_bytes, flag, scan, (int)nf_all, st));
    unsigned tail[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(&tail[0], flag + (nf_all - 1), sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&tail[1], scan + (nf_all - 1), sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    const uint64_t F = (uint64_t)tail[0] + tail[1];
    HIP_TRY(c, b->face_nodes.alloc((size_t)F * t.nfn));
    HIP_TRY(c, b->cells.alloc((size_t)F));
    HIP_TRY(c, b->local_faces.alloc((size_t)F));
    if (F) {
        dispatch(face_node_counts, t.nfn, 0, [&](auto nfn) {
            hipLaunchKernelGGL(k_face_emit<nfn()>, dim3(grid), dim3(256), 0, st, c->conn.p, n, t, nf_all, keys.p, vals.p, flag, scan, b->face_nodes.p,
                               b->cells.p, b->local_faces.p);
            return 0;
        });
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipStreamSynchronize(st));   // the scratch is released on return
    b->num_faces = F;
    b->has_faces = true;
    b->has_verts = b->has_cells = false;
    c->last_kernel = "k_face_keys + radix sort + k_face_unique + scan + k_face_emit";
    return FH_OK;
}

// the sorted, unique members of a u64 id list over [0, domain)
static int compact_ids(fh_ctx* c, const unsigned long long* ids, size_t count, size_t domain, DevBuf<unsigned long long>& out, uint64_t& nout) {
    hipStream_t st = c->stream;
    nout = 0;
    if (count == 0 || domain == 0) return FH_OK;
    DevBuf<unsigned> flag, scan;
    DevBuf<char> tmp;
    HIP_TRY(c, flag.alloc(domain));
    HIP_TRY(c, scan.alloc(domain));
    HIP_TRY(c, hipMemsetAsync(flag.p, 0, sizeof(unsigned) * domain, st));
    hipLaunchKernelGGL(k_mark_ids, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, ids, count, flag.p);
    HIP_TRY(c, hipGetLastError());
    size_t scan_bytes = 0;
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, flag.p, scan.p, (int)domain, st));
    HIP_TRY(c, tmp.alloc(scan_bytes));
    HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(tmp.p, scan_bytes, flag.p, scan.p, (int)domain, st));
    unsigned tail[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(&tail[0], flag.p + (domain - 1), sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&tail[1], scan.p + (domain - 1), sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    nout = (uint64_t)tail[0] + tail[1];
    HIP_TRY(c, out.alloc((size_t)nout));
    hipLaunchKernelGGL(k_compact_flagged, dim3((unsigned)((domain + 255) / 256)), dim3(256), 0, st, flag.p, scan.p, domain, out.p);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(st));
    return FH_OK;
}

static int two_phase(fh_ctx* c, const DevBuf<unsigned long long>& list, uint64_t n, uint64_t* count, uint64_t* out) {
    if (count) *count = n;
    if (out && n) {
        HIP_TRY(c, hipMemcpyAsync(out, list.p, sizeof(uint64_t) * n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return FH_OK;
}

// ---- surface load ---------------------------------------------------------------------------------------------------------------
// the face-point records of a rule: the face point mapped into the cell by the affine map through the face's corners, the engine's
// reference basis and gradients there
static int ensure_face_records(fh_ctx* c, const double* weights, const double* points, uint32_t nq) {
    BoundaryStore* b = store(c);
    const FaceTable& t = face_table(c->elem_kind);
    const int D = c->ei.d, fd = D - 1, NG = c->ei.ng, gk = c->ei.geom_kind;
    if (b->has_recs && b->rule_w.size() == nq && std::equal(weights, weights + nq, b->rule_w.begin()) &&
        std::equal(points, points + (size_t)nq * fd, b->rule_pts.begin()))
        return FH_OK;
    b->has_recs = false;
    std::vector<FacePointRec> recs((size_t)t.nfaces * nq);
    std::vector<double> phi((size_t)c->ei.n), pg(8), gg(24);
    const bool tri_face = (gk == FH_TET4);
    for (int lf = 0; lf < t.nfaces; ++lf) {
        // corners of the face in the face's node list: the first and the last node of a segment, the first 3 / 4 of a triangle / quadrilateral
        double cr[4][3] = {{0}};
        const int ncorn = (D == 2) ? 2 : (tri_face ? 3 : 4);
        for (int k = 0; k < ncorn; ++k) {
            const int m = (D == 2) ? (k == 0 ? 0 : t.nfn - 1) : k;
            corner_ref(gk, t.nodes[lf][m], cr[k]);
        }
        double ts[3] = {0, 0, 0}, tt[3] = {0, 0, 0}, nref[3] = {0, 0, 0};
        const int last = (D == 2) ? 1 : (tri_face ? 2 : 3);
        for (int k = 0; k < D; ++k) { ts[k] = 0.5 * (cr[1][k] - cr[0][k]); tt[k] = 0.5 * (cr[last][k] - cr[0][k]); }
        if (D == 2) { nref[0] = ts[1]; nref[1] = -ts[0]; }
        else {
            nref[0] = ts[1] * tt[2] - ts[2] * tt[1];
            nref[1] = ts[2] * tt[0] - ts[0] * tt[2];
            nref[2] = ts[0] * tt[1] - ts[1] * tt[0];
        }
        for (uint32_t q = 0; q < nq; ++q) {
            FacePointRec& r = recs[(size_t)lf * nq + q];
            std::memset(&r, 0, sizeof r);
            const double s = points[(size_t)q * fd], tq = fd > 1 ? points[(size_t)q * fd + 1] : 0.0;
            double xi[3] = {0, 0, 0};
            for (int k = 0; k < D; ++k) xi[k] = cr[0][k] + ts[k] * (s + 1.0) + (D == 3 ? tt[k] * (tq + 1.0) : 0.0);
            ref_basis(c->elem_kind, xi, phi.data());
            ref_basis(gk, xi, pg.data());
            ref_gradients(gk, xi, gg.data());
            for (int a = 0; a < NG; ++a) {
                r.PG[a] = pg[a];
                for (int k = 0; k < D; ++k) r.G[a][k] = gg[(size_t)D * a + k];
            }
            for (int m = 0; m < t.nfn; ++m) r.NF[m] = phi[t.nodes[lf][m]];
            for (int k = 0; k < 3; ++k) r.nref[k] = nref[k];
        }
    }
    HIP_TRY(c, b->recs.alloc(recs.size()));
    HIP_TRY(c, b->w.alloc(nq));
    HIP_TRY(c, hipMemcpyAsync(b->recs.p, recs.data(), sizeof(FacePointRec) * recs.size(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(b->w.p, weights, sizeof(double) * nq, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    b->rule_w.assign(weights, weights + nq);
    b->rule_pts.assign(points, points + (size_t)nq * fd);
    b->has_recs = true;
    return FH_OK;
}

// node -> (position in the list, face node) adjacency of a face list, built once per list (the key: its length and a fingerprint of its
// contents) and checked while it is built
static int ensure_face_adjacency(fh_ctx* c, const unsigned long long* cells_dev, const unsigned* lf_dev, uint64_t F, const char* who) {
    BoundaryStore* b = store(c);
    const FaceTable& t = face_table(c->elem_kind);
    hipStream_t st = c->stream;
    if (F * (uint64_t)t.nfn >= (1ull << 31)) return c->fail(FH_UNSUPPORTED, std::string(who) + ": num_faces * nodes per face must be < 2^31");
    if (b->hash_tmp.n < F) HIP_TRY(c, b->hash_tmp.alloc((size_t)F));
    if (!b->hash_out.p) HIP_TRY(c, b->hash_out.alloc(1));
    size_t red_bytes = 0;
    HIP_TRY(c, hipcub::DeviceReduce::Sum(nullptr, red_bytes, b->hash_tmp.p, b->hash_out.p, (int)F, st));
    if (b->hash_cub.n < red_bytes) HIP_TRY(c, b->hash_cub.alloc(red_bytes));
    const unsigned gf = (unsigned)((F + 255) / 256);
    hipLaunchKernelGGL(k_surface_list_hash, dim3(gf), dim3(256), 0, st, cells_dev, lf_dev, (unsigned long long)F, b->hash_tmp.p);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipcub::DeviceReduce::Sum(b->hash_cub.p, red_bytes, b->hash_tmp.p, b->hash_out.p, (int)F, st));
    unsigned long long h = 0;
    HIP_TRY(c, hipMemcpyAsync(&h, b->hash_out.p, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (b->has_adj && b->adj_faces == F && b->adj_hash == h) return FH_OK;
    b->has_adj = false;
    const size_t ne = (size_t)F * t.nfn;
    DevBuf<unsigned> node_in, ent_in;
    DevBuf<int> bad;
    DevBuf<char> tmp;
    HIP_TRY(c, node_in.alloc(ne));
    HIP_TRY(c, ent_in.alloc(ne));
    HIP_TRY(c, b->ent_node.alloc(ne));
    HIP_TRY(c, b->ent.alloc(ne));
    HIP_TRY(c, bad.alloc(1));
    HIP_TRY(c, hipMemsetAsync(bad.p, 0, sizeof(int), st));
    hipLaunchKernelGGL(k_surface_entries, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, c->conn.p, c->ei.n, t, cells_dev, lf_dev,
                       (unsigned long long)F, (unsigned long long)c->E, node_in.p, ent_in.p, bad.p);
    HIP_TRY(c, hipGetLastError());
    int bits = 1;
    while ((1ull << bits) < c->N) ++bits;
    size_t sort_bytes = 0;
    HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, node_in.p, b->ent_node.p, ent_in.p, b->ent.p, (int)ne, 0, bits, st));
    HIP_TRY(c, tmp.alloc(sort_bytes));
    HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(tmp.p, sort_bytes, node_in.p, b->ent_node.p, ent_in.p, b->ent.p, (int)ne, 0, bits, st));   // stable: positions ascending per node
    int hb = 0;
    HIP_TRY(c, hipMemcpyAsync(&hb, bad.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    if (hb) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": a cell or local face index of the face list is out of range");
    b->adj_faces = F;
    b->adj_hash = h;
    b->adj_entries = ne;
    b->has_adj = true;
    return FH_OK;
}

static int surface_ready(fh_ctx* c, const char* who, const void* cells, const void* lfs, uint64_t F, const double* points, uint32_t nq) {
    int rc = boundary_ready(c, who);
    if (rc) return rc;
    if (face_table(c->elem_kind).nfaces == 0) return c->fail(FH_UNSUPPORTED, std::string(who) + ": this element kind has no faces");
    if (nq == 0 || !points) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": no face rule given");
    if (F && (!cells || !lfs)) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null face list");
    return FH_OK;
}

static void fill_surface_args(fh_ctx* c, SurfaceArgs& a, const uint64_t* cells_dev, const uint32_t* lf_dev, uint64_t F, uint32_t nq) {
    a.verts = c->verts.p;
    a.conn = c->conn.p;
    a.cells = reinterpret_cast<const unsigned long long*>(cells_dev);
    a.local_faces = lf_dev;
    a.num_faces = F;
    a.E = c->E;
    a.n = c->ei.n;
    a.nq = (int)nq;
    a.w = c->bnd->w.p;
    a.recs = c->bnd->recs.p;
}

extern "C" {

int fh_find_boundary_faces(fh_ctx* c, uint64_t* num_faces, uint32_t* nodes_per_face) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int rc = boundary_ready(c, "fh_find_boundary_faces");
    if (rc) return rc;
    rc = find_boundary_faces(c);
    if (rc) return rc;
    if (num_faces) *num_faces = c->bnd->num_faces;
    if (nodes_per_face) *nodes_per_face = (uint32_t)c->bnd->nfn;
    return FH_OK;
}

int fh_boundary_faces_dev(fh_ctx* c, uint64_t* face_nodes_dev, uint64_t* cells_dev, uint32_t* local_faces_dev) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int rc = boundary_ready(c, "fh_boundary_faces");
    if (rc) return rc;
    rc = find_boundary_faces(c);
    if (rc) return rc;
    const BoundaryStore* b = c->bnd;
    const size_t F = (size_t)b->num_faces;
    if (F == 0) return FH_OK;
    if (face_nodes_dev) HIP_TRY(c, hipMemcpyAsync(face_nodes_dev, b->face_nodes.p, sizeof(uint64_t) * F * b->nfn, hipMemcpyDeviceToDevice, c->stream));
    if (cells_dev) HIP_TRY(c, hipMemcpyAsync(cells_dev, b->cells.p, sizeof(uint64_t) * F, hipMemcpyDeviceToDevice, c->stream));
    if (local_faces_dev) HIP_TRY(c, hipMemcpyAsync(local_faces_dev, b->local_faces.p, sizeof(uint32_t) * F, hipMemcpyDeviceToDevice, c->stream));
    return FH_OK;
}

int fh_boundary_faces(fh_ctx* c, uint64_t* face_nodes, uint64_t* cells, uint32_t* local_faces) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int rc = boundary_ready(c, "fh_boundary_faces");
    if (rc) return rc;
    rc = find_boundary_faces(c);
    if (rc) return rc;
    const BoundaryStore* b = c->bnd;
    const size_t F = (size_t)b->num_faces;
    if (F == 0) return FH_OK;
    if (face_nodes) HIP_TRY(c, hipMemcpyAsync(face_nodes, b->face_nodes.p, sizeof(uint64_t) * F * b->nfn, hipMemcpyDeviceToHost, c->stream));
    if (cells) HIP_TRY(c, hipMemcpyAsync(cells, b->cells.p, sizeof(uint64_t) * F, hipMemcpyDeviceToHost, c->stream));
    if (local_faces) HIP_TRY(c, hipMemcpyAsync(local_faces, b->local_faces.p, sizeof(uint32_t) * F, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FH_OK;
}

int fh_boundary_vertices(fh_ctx* c, uint64_t* count, uint64_t* nodes) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int rc = boundary_ready(c, "fh_boundary_vertices");
    if (rc) return rc;
    rc = find_boundary_faces(c);
    if (rc) return rc;
    BoundaryStore* b = c->bnd;
    if (!b->has_verts) {
        rc = compact_ids(c, b->face_nodes.p, (size_t)b->num_faces * b->nfn, (size_t)c->N, b->bverts, b->num_verts);
        if (rc) return rc;
        b->has_verts = true;
    }
    return two_phase(c, b->bverts, b->num_verts, count, nodes);
}

int fh_boundary_cells(fh_ctx* c, uint64_t* count, uint64_t* cells) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int rc = boundary_ready(c, "fh_boundary_cells");
    if (rc) return rc;
    rc = find_boundary_faces(c);
    if (rc) return rc;
    BoundaryStore* b = c->bnd;
    if (!b->has_cells) {
        rc = compact_ids(c, b->cells.p, (size_t)b->num_faces, (size_t)c->E, b->bcells, b->num_cells);
        if (rc) return rc;
        b->has_cells = true;
    }
    return two_phase(c, b->bcells, b->num_cells, count, cells);
}

int fh_boundary_search_scratch_bytes(const fh_ctx* c, uint64_t* bytes) {
    if (!c || !bytes) return FH_BAD_ARGUMENT;
    *bytes = (c->bnd && c->bnd->has_faces) ? c->bnd->scratch_bytes : 0;
    return FH_OK;
}

int fh_assemble_surface_load_dev(fh_ctx* c, int load_kind, uint32_t sdim, const uint64_t* cells_dev, const uint32_t* local_faces_dev, uint64_t F,
                                 const double* weights, const double* points, uint32_t nq, const double* data_dev, uint64_t data_count,
                                 double* out_dev) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    const char* who = "fh_assemble_surface_load";
    int rc = surface_ready(c, who, cells_dev, local_faces_dev, F, points, nq);
    if (rc) return rc;
    const int D = c->ei.d;
    if (!weights) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": no weights given");
    if (!out_dev) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": out is null");
    if (load_kind != FH_LOAD_TRACTION && load_kind != FH_LOAD_PRESSURE) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": unknown load kind");
    if (load_kind == FH_LOAD_PRESSURE && (int)sdim != D) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": a pressure load needs solution dim == geometry dim");
    if (sdim != 1 && (int)sdim != D) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": solution dim must be 1 or the geometry dim");
    if (!data_dev) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": no load data given");
    int mode;
    if (data_count == 1) mode = 0;
    else if (data_count == F) mode = 1;
    else if (data_count == F * (uint64_t)nq) mode = 2;
    else return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": data_count must be 1, num_faces or num_faces * nq");
    if (F == 0) return FH_OK;
    rc = ensure_face_records(c, weights, points, nq);
    if (rc) return rc;
    rc = ensure_face_adjacency(c, reinterpret_cast<const unsigned long long*>(cells_dev), local_faces_dev, F, who);
    if (rc) return rc;
    BoundaryStore* b = c->bnd;
    SurfaceArgs a{};
    fill_surface_args(c, a, cells_dev, local_faces_dev, F, nq);
    a.sdim = (int)sdim;
    a.pressure = load_kind == FH_LOAD_PRESSURE;
    a.data = data_dev;
    a.data_mode = mode;
    a.out = out_dev;
    const unsigned grid = (unsigned)((b->adj_entries + 255) / 256);
    dispatch_or_last(low_order_kinds, c->ei.geom_kind, [&](auto gk) {
        hipLaunchKernelGGL((k_surface_load<kind_geom<gk()>::D, kind_geom<gk()>::NG>), dim3(grid), dim3(256), 0, c->stream, a, face_table(c->elem_kind).nfn,
                           b->ent_node.p, b->ent.p, (size_t)b->adj_entries);
        return 0;
    });
    HIP_TRY(c, hipGetLastError());
    c->last_kernel = "k_surface_load";
    return FH_OK;
}

int fh_assemble_surface_load(fh_ctx* c, int load_kind, uint32_t sdim, const uint64_t* cells, const uint32_t* local_faces, uint64_t F,
                             const double* weights, const double* points, uint32_t nq, const double* data, uint64_t data_count, double* out) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    const char* who = "fh_assemble_surface_load";
    int rc = surface_ready(c, who, cells, local_faces, F, points, nq);
    if (rc) return rc;
    if (!out) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": out is null");
    if (!data) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": no load data given");
    if (sdim != 1 && (int)sdim != c->ei.d) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": solution dim must be 1 or the geometry dim");
    const size_t len = (size_t)sdim * c->N, comps = load_kind == FH_LOAD_PRESSURE ? 1 : sdim, nd = (size_t)data_count * comps;
    DevBuf<double> d, v;
    DevBuf<unsigned long long> cd;
    DevBuf<unsigned> ld;
    HIP_TRY(c, d.alloc(len));
    HIP_TRY(c, v.alloc(nd));
    HIP_TRY(c, cd.alloc((size_t)F));
    HIP_TRY(c, ld.alloc((size_t)F));
    HIP_TRY(c, hipMemcpyAsync(d.p, out, sizeof(double) * len, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(v.p, data, sizeof(double) * nd, hipMemcpyHostToDevice, c->stream));
    if (F) {
        HIP_TRY(c, hipMemcpyAsync(cd.p, cells, sizeof(uint64_t) * F, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(ld.p, local_faces, sizeof(uint32_t) * F, hipMemcpyHostToDevice, c->stream));
    }
    rc = fh_assemble_surface_load_dev(c, load_kind, sdim, reinterpret_cast<const uint64_t*>(cd.p), ld.p, F, weights, points, nq, v.p, data_count, d.p);
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    HIP_TRY(c, hipMemcpyAsync(out, d.p, sizeof(double) * len, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FH_OK;
}

int fh_physical_face_quadrature_points_dev(fh_ctx* c, const uint64_t* cells_dev, const uint32_t* local_faces_dev, uint64_t F, const double* points,
                                           uint32_t nq, double* x_dev) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    const char* who = "fh_physical_face_quadrature_points";
    int rc = surface_ready(c, who, cells_dev, local_faces_dev, F, points, nq);
    if (rc) return rc;
    if (!x_dev) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": output is null");
    if (F == 0) return FH_OK;
    // the weights do not enter: keep the ones of a cached rule with the same points, ones otherwise
    BoundaryStore* b = store(c);
    const size_t np = (size_t)nq * (c->ei.d - 1);
    std::vector<double> w(nq, 1.0);
    if (b->has_recs && b->rule_w.size() == nq && std::equal(points, points + np, b->rule_pts.begin())) w = b->rule_w;
    rc = ensure_face_records(c, w.data(), points, nq);
    if (rc) return rc;
    rc = ensure_face_adjacency(c, reinterpret_cast<const unsigned long long*>(cells_dev), local_faces_dev, F, who);   // (checks the list)
    if (rc) return rc;
    SurfaceArgs a{};
    fill_surface_args(c, a, cells_dev, local_faces_dev, F, nq);
    const unsigned grid = (unsigned)((F * nq + 255) / 256);
    dispatch_or_last(low_order_kinds, c->ei.geom_kind, [&](auto gk) {
        hipLaunchKernelGGL((k_face_physical_points<kind_geom<gk()>::D, kind_geom<gk()>::NG>), dim3(grid), dim3(256), 0, c->stream, a, x_dev);
        return 0;
    });
    HIP_TRY(c, hipGetLastError());
    return FH_OK;
}

int fh_physical_face_quadrature_points(fh_ctx* c, const uint64_t* cells, const uint32_t* local_faces, uint64_t F, const double* points, uint32_t nq,
                                       double* x) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    const char* who = "fh_physical_face_quadrature_points";
    int rc = surface_ready(c, who, cells, local_faces, F, points, nq);
    if (rc) return rc;
    if (!x) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": output is null");
    if (F == 0) return FH_OK;
    const size_t n = (size_t)F * nq * c->ei.d;
    DevBuf<double> d;
    DevBuf<unsigned long long> cd;
    DevBuf<unsigned> ld;
    HIP_TRY(c, d.alloc(n));
    HIP_TRY(c, cd.alloc((size_t)F));
    HIP_TRY(c, ld.alloc((size_t)F));
    HIP_TRY(c, hipMemcpyAsync(cd.p, cells, sizeof(uint64_t) * F, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(ld.p, local_faces, sizeof(uint32_t) * F, hipMemcpyHostToDevice, c->stream));
    rc = fh_physical_face_quadrature_points_dev(c, reinterpret_cast<const uint64_t*>(cd.p), ld.p, F, points, nq, d.p);
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    HIP_TRY(c, hipMemcpyAsync(x, d.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FH_OK;
}

}  // extern "C"
