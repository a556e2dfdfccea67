// The host side of every element-to-node pass, and its C ABI: the residual (fh_assemble_vector), the source vector and the physical quadrature
// points, the energy (fh_assemble_scalar), the matrix-free operator and tangent y = T(u) x with their diagonal and Dirichlet rows, the mass
// term and the shifted map alpha M + beta T(u), and the Newton residual.  The steps they share are written once, in "the host frame" below:
// the arguments of a whole-table pass, whether the element tiles serve a call and where their partials go, the ordered single-table pass
// (tiles, else element vectors and ordered node sums), and the walk over the groups of a rule-set table.
#include "engine_internal.hpp"

// with_expansion(OP, a, f): f(true_type) when the arguments carry the per-element expansion (a.theta) and OP has such kernels, f(false_type)
// while none is set; -1 for an operator without them (the entry points refuse it before any launch)
template <int OP, class F>
static int with_expansion(const KArgs& a, F&& f) {
    return dispatch_bool(a.theta != nullptr, [&](auto ex) {
        if constexpr (!ex() || op_expands(OP)) return f(ex);
        else return -1;
    });
}
template <int EK, int OP>
static int launch_vector(fh_ctx* c, KArgs& a, size_t lds, int grid) {
    return with_expansion<OP>(a, [&](auto ex) { return launch_lds(c, k_assemble_vector<EK, OP, ex()>, dim3(grid), dim3(256), lds, c->stream, a); });
}
template <int EK, int OP, int NT>
static int launch_vector_stream_nt(fh_ctx* c, KArgs& a) {
    constexpr int EPB = NT / ElemT<EK>::N;
    const size_t lds = make_layout<EK, OP, WHAT_VECTOR>(a.nq, EPB, 0, 0, false, 0, 1).bytes();
    if (lds > LDS_TARGET + 8 * 1024) return -1;
    const long long nbatch = (a.work_end - a.work_begin + EPB - 1) / EPB;
    const int per_cu = std::max(1, (int)std::min<size_t>(c->opt.VEC_WGS_PER_CU.value_or(3), (LDS_LIMIT - 512) / std::max<size_t>(lds, 1)));
    const int grid = std::max(1, (int)std::min<long long>(nbatch, (long long)c->opt.PIPE_GRID.value_or(c->num_cus * per_cu)));   // (tests force many batches per workgroup)
    return with_expansion<OP>(a, [&](auto ex) { return launch_lds(c, k_assemble_vector_stream<EK, OP, NT, ex()>, dim3(grid), dim3(NT), lds, c->stream, a); });
}
template <int EK, int OP>
static int launch_vector_stream(fh_ctx* c, KArgs& a) {
    if constexpr (ElemT<EK>::NG == ElemT<EK>::N && (ElemT<EK>::N == 4 || ElemT<EK>::N == 8)) {
        int rs = launch_vector_stream_nt<EK, OP, 256>(c, a);
        if (rs < 0) rs = launch_vector_stream_nt<EK, OP, 128>(c, a);
        return rs;
    } else {
        return -1;
    }
}
template <int EK, int OP>
static int launch_scalar(fh_ctx* c, KArgs& a, size_t lds, int grid) {
    return with_expansion<OP>(a, [&](auto ex) { return launch_lds(c, k_assemble_scalar<EK, OP, ex()>, dim3(grid), dim3(256), lds, c->stream, a); });
}

// register-resident element pass (element_pass.hpp): one thread per element of the small iso-parametric kinds, operators with a
// vector / scalar form.  Returns -1 when the combination is not covered (the callers keep the staged kernels).
template <int WHAT>
static int launch_element_pass(fh_ctx* c, KArgs& a) {
    const int grid = (int)((a.num_elements + 255) / 256);
    return dispatch(low_order_kinds, c->elem_kind, elliptic_ops, c->op, -1, [&](auto ek, auto op) {
        return with_expansion<op()>(a, [&](auto ex) {
            hipLaunchKernelGGL((k_element_pass<ek(), op(), WHAT, ex()>), dim3(grid), dim3(256), 0, c->stream, a);
            HIP_TRY(c, hipGetLastError());
            return (int)FH_OK;
        });
    });
}
static int launch_vector_from_elements_soa(fh_ctx* c, int sdim, const double* fe, double* out_dev, const unsigned* adj_off = nullptr,
                                           const unsigned* adj = nullptr, const SourceG* scaled = nullptr) {
    const int grid = (int)(((long long)c->N + 255) / 256);
    if (!adj_off) { adj_off = c->n2e_off.p; adj = c->n2e.p; }
    return dispatch_or_last(solution_dims, sdim, [&](auto s) {
        if (scaled)   // scalar entries, sdim components g[c] sum
            hipLaunchKernelGGL((k_vector_from_elements_soa<1, s()>), dim3(grid), dim3(256), 0, c->stream, (int)c->N, c->ei.n, (long long)c->E, adj_off, adj, fe,
                               out_dev, *scaled);
        else
            hipLaunchKernelGGL((k_vector_from_elements_soa<s(), 0>), dim3(grid), dim3(256), 0, c->stream, (int)c->N, c->ei.n, (long long)c->E, adj_off, adj, fe,
                               out_dev);
        HIP_TRY(c, hipGetLastError());
        return (int)FH_OK;
    });
}
// ... of the element vectors in c->fe_scratch, one thread per row over the pattern's adjacency
static int launch_vector_from_elements(fh_ctx* c, int sdim, double* out_dev) {
    const int grid = (int)(((long long)c->N * sdim + 255) / 256);
    return dispatch_or_last(solution_dims, sdim, [&](auto s) {
        hipLaunchKernelGGL(k_vector_from_elements<s()>, dim3(grid), dim3(256), 0, c->stream, (int)c->N, c->n2e_off.p, c->n2e.p, c->fe_scratch.p, out_dev);
        HIP_TRY(c, hipGetLastError());
        return (int)FH_OK;
    });
}
static bool element_pass_covers(const fh_ctx* c) {
    return !c->ragged && !c->opt.NO_ELEMENT_PASS &&
           (c->elem_kind == FH_HEX8 || c->elem_kind == FH_TET4 || c->elem_kind == FH_QUAD4 || c->elem_kind == FH_TRI3);
}
// the element tiles (vector_tiles.hip) serve this context
bool tiles_enabled(const fh_ctx* c) { return element_pass_covers(c) && !c->opt.VECTOR_ATOMICS && !c->opt.NO_VECTOR_TILES; }

// ---- the host frame of the element-to-node passes
// the arguments of a pass over the whole table: every element, or the active ones of an element mask, in the mesh's order (no element list)
KArgs pass_args(fh_ctx* c) {
    KArgs a;
    fill_common(c, a);
    a.work_begin = 0;
    a.work_end = (long long)(c->has_mask ? c->num_active : c->E);
    a.labels = nullptr;
    return a;
}
// the element mask for the kernels that visit every element and zero the inactive ones' contributions, and the list of the active elements
// for the assembled routes that visit only those (a.labels: asked for where such a route is taken)
const unsigned char* active_mask(const fh_ctx* c) { return c->has_mask ? c->active.p : nullptr; }
static const unsigned* active_labels(const fh_ctx* c) { return c->has_mask ? c->active_list.p : nullptr; }

// *serve: the element tiles (vector_tiles.hip) serve this context -- the switches leave them on, and the tables are built for its topology (they
// could not be: vt_bad) -- and `part` then holds comps doubles per tile partial (comps 0: the caller sizes a buffer of another shape).  The
// buffer is the caller's: fe_scratch, the Newton solver's and the integrators' partials are read by one pass while another is written.
// even_with_atomics: the energy's condition -- a sum of partials whatever VECTOR_ATOMICS says, so that switch leaves it on the tiles.
int tile_partials(fh_ctx* c, DevBuf<double>& part, int comps, bool* serve, bool even_with_atomics) {
    *serve = false;
    if (!(even_with_atomics ? element_pass_covers(c) && !c->opt.NO_VECTOR_TILES : tiles_enabled(c))) return FH_OK;
    const int rc = ensure_vector_tiles(c);
    if (rc || c->vt_bad) return rc;
    const size_t need = (size_t)c->vt.v.npartials * comps;
    if (part.n < need) HIP_TRY(c, part.alloc(need));
    *serve = true;
    return FH_OK;
}

// one quadrature table (or one group of a rule-set table) ADDED to out (S N doubles) without atomics: tile(a, &done) leaves its partials in
// c->fe_scratch where the tiles cover the pass and the tiles' node pass sums them (tile nullptr: the caller owns that branch); else
// elem(a, active, fe) leaves the element vectors fe[a][e][c] in c->fe_scratch and one thread per node sums its (element, local node) entries
// of the source adjacency in order.  The status slot is the caller's.
template <class Tile, class Elem>
static int ordered_single(fh_ctx* c, double* out, Tile&& tile, Elem&& elem) {
    const int S = c->S();
    KArgs a = pass_args(c);
    if constexpr (!std::is_null_pointer_v<std::decay_t<Tile>>) {
        bool done;
        const int rc = tile(a, &done);
        if (rc) return rc;
        if (done) {
            HIP_TRY(c, vector_tiles_node_pass(c->stream, S, (int)c->N, c->vt.v, c->fe_scratch.p, out));
            return FH_OK;
        }
    }
    int rc = build_source_adjacency(c);
    if (rc) return rc;
    const size_t need = (size_t)c->E * c->ei.n * S;
    if (c->fe_scratch.n < need) HIP_TRY(c, c->fe_scratch.alloc(need));
    rc = elem(a, active_mask(c), c->fe_scratch.p);
    if (rc) return rc;
    HIP_TRY(c, hipGetLastError());
    return launch_vector_from_elements_soa(c, S, c->fe_scratch.p, out, c->src_n2e_off.p, c->src_n2e.p);
}

// out (n doubles) zeroed, then single(failed) of the one table, or of every group of a rule-set table, accumulating into it
template <class F>
static int walk_groups_into(fh_ctx* c, double* out, size_t n, uint64_t* failed, F&& single) {
    HIP_TRY(c, hipMemsetAsync(out, 0, sizeof(double) * n, c->stream));
    return c->rs.active ? rs_walk_accumulating(c, failed, single) : single(failed);
}

// the host-array form of a device entry point: a device buffer of len (+ pad) doubles, `host` copied in (copy_in), run(buffer), the buffer
// copied back and the stream waited for (the buffer is released on return)
template <class Run>
static int through_device(fh_ctx* c, double* host, size_t len, size_t pad, bool copy_in, Run&& run) {
    DevBuf<double> d;
    HIP_TRY(c, d.alloc(len + pad));
    if (copy_in) HIP_TRY(c, hipMemcpyAsync(d.p, host, sizeof(double) * len, hipMemcpyHostToDevice, c->stream));
    const int rc = run(d.p);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(host, d.p, sizeof(double) * len, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FH_OK;
}

extern "C" {

static int assemble_vector_single(fh_ctx* c, double* out_dev, uint64_t* failed);
int fh_assemble_vector_dev(fh_ctx* c, double* out_dev, uint64_t* failed) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (op_has_stress(c->op)) {
        const int rb = expansion_blocked(c, "fh_assemble_vector");
        if (rb) return rb;
    }
    if (!c->rs.active) return assemble_vector_single(c, out_dev, failed);
    return rs_walk_accumulating(c, failed, [&](uint64_t* f) { return assemble_vector_single(c, out_dev, f); });
}
int fh_assemble_vector_async_dev(fh_ctx* c, double* out_dev) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    // nothing is read back between the groups of a rule-set table here, so a per-group reset would erase what an earlier group
    // reported: one reset in front of the walk (the device keeps the lowest failing element over all launches since the reset)
    if (c->rs.active) {
        const int r0 = reset_status(c);
        if (r0) return r0;
        c->keep_status = true;
    }
    c->defer_status = true;
    const int rc = fh_assemble_vector_dev(c, out_dev, nullptr);
    c->defer_status = false;
    c->keep_status = false;
    return rc;
}
// element tiles of the residual / source vector passes (vector_tiles.hip): once per mesh topology
extern "C++" int ensure_vector_tiles(fh_ctx* c) {
    if (c->vt_gen == c->topo_gen) return FH_OK;
    int bad = 0;
    const hipError_t e = vector_tiles_build(c->stream, c->conn.p, c->ei.n, (long long)c->E, c->verts.p, c->ei.d, (int)c->N, &c->vt, &bad);
    if (e == hipErrorOutOfMemory) {   // no room for the tables: the callers keep the two-pass kernels
        (void)hipGetLastError();
        c->vt.release();
        bad = 1;
    } else {
        HIP_TRY(c, e);
    }
    c->vt_bad = bad != 0;
    c->vt_gen = c->topo_gen;
    return FH_OK;
}
int fh_vector_tiles_stats(fh_ctx* c, uint64_t* tiles, uint64_t* partials, uint64_t* max_tile_nodes, uint64_t* max_node_partials) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (!c->has_mesh) return c->fail(FH_INVALID_STATE, "fh_vector_tiles_stats: no finite element mesh set");
    if (!element_pass_covers(c) || c->opt.NO_VECTOR_TILES) return c->fail(FH_UNSUPPORTED, "fh_vector_tiles_stats: this mesh has no element tiles");
    const int rc = ensure_vector_tiles(c);
    if (rc) return rc;
    if (c->vt_bad) return c->fail(FH_UNSUPPORTED, "fh_vector_tiles_stats: the element tiles could not be built for this mesh");
    unsigned mt = 0, mp = 0;
    HIP_TRY(c, vector_tiles_stats(c->stream, c->vt.v, (int)c->N, &mt, &mp));
    if (tiles) *tiles = (uint64_t)c->vt.v.ntiles;
    if (partials) *partials = c->vt.v.npartials;
    if (max_tile_nodes) *max_tile_nodes = mt;
    if (max_node_partials) *max_node_partials = mp;
    return FH_OK;
}
static int assemble_vector_single(fh_ctx* c, double* out_dev, uint64_t* failed) {
    int rc = check_ready(c, "fh_assemble_vector", false);
    if (rc) return rc;
    if (!op_has_stress(c->op)) return c->fail(FH_UNSUPPORTED, "fh_assemble_vector: the mass assembler has no vector form");
    if (!out_dev) return c->fail(FH_BAD_ARGUMENT, "fh_assemble_vector: out is null");
    rc = c->keep_status ? FH_OK : reset_status(c);
    if (rc) return rc;
    if (c->E == 0) return FH_OK;
    KArgs a = pass_args(c);
    a.vec_out = out_dev;
    if (a.work_end == 0) return read_status(c, failed);
    // small iso-parametric elements: tiles of 256 elements, one thread per element, the tile's distinct nodes summed in LDS, only
    // those partial sums through HBM, then one thread per node (vector_tiles.hip); no atomics, bitwise reproducible; an element mask
    // zeroes the contributions of the inactive elements
    bool serve;
    rc = tile_partials(c, c->fe_scratch, c->S(), &serve);
    if (rc) return rc;
    if (serve && vector_tiles_element_pass(c->elem_kind, c->op, c->stream, a, c->vt.v, active_mask(c), c->fe_scratch.p) == FH_OK) {
        HIP_TRY(c, hipGetLastError());
        c->last_kernel = "k_element_pass_tiled + k_vector_from_partials";
        HIP_TRY(c, vector_tiles_node_pass(c->stream, c->S(), (int)c->N, c->vt.v, c->fe_scratch.p, out_dev));
        return read_status(c, failed);
    }
    a.labels = active_labels(c);   // (the routes below take an element list where they can, and say where they cannot)
    // small iso-parametric elements without an element list: one thread per element, element vectors laid out by local node, then
    // one thread per node (element_pass.hpp); no atomics, bitwise reproducible
    if (!a.labels && element_pass_covers(c) && !c->opt.VECTOR_ATOMICS) {
        rc = build_pattern(c);  // the node -> (element, local node) adjacency comes with the pattern
        if (rc) return rc;
        const size_t need = (size_t)c->E * c->ei.n * c->S();
        if (c->fe_scratch.n < need) HIP_TRY(c, c->fe_scratch.alloc(need));
        a.ke_out = c->fe_scratch.p;
        const int rs = launch_element_pass<EP_VECTOR>(c, a);
        if (rs == FH_OK) {
            c->last_kernel = "k_element_pass + k_vector_from_elements_soa";
            rc = launch_vector_from_elements_soa(c, c->S(), c->fe_scratch.p, out_dev);
            if (rc) return rc;
            return read_status(c, failed);
        }
        if (rs > 0) return rs;
        a.ke_out = nullptr;
    }
    // persistent, prefetching form for the small iso-parametric elements (no element list: a mask keeps the generic kernel).
    // Two passes by default: element vectors to a scratch buffer, then one thread per row sums its node's entries in
    // ascending element order -- no atomics, bitwise reproducible (FENRIS_HIP_VECTOR_ATOMICS keeps the one-pass scatter)
    if (!a.labels) {
        const bool two_pass = !c->opt.VECTOR_ATOMICS && !c->ragged &&
                              (c->elem_kind == FH_HEX8 || c->elem_kind == FH_TET4 || c->elem_kind == FH_QUAD4);
        if (two_pass) {
            rc = build_pattern(c);  // the node -> (element, local node) adjacency comes with the pattern
            if (rc) return rc;
            const size_t need = (size_t)c->E * c->ei.n * c->S();
            if (c->fe_scratch.n < need) HIP_TRY(c, c->fe_scratch.alloc(need));
            a.ke_out = c->fe_scratch.p;
        }
        const int rs = dispatch(all_kinds, c->elem_kind, elliptic_ops, c->op, -1, [&](auto ek, auto op) { return launch_vector_stream<ek(), op()>(c, a); });
        if (rs == FH_OK && two_pass) {
            rc = launch_vector_from_elements(c, c->S(), out_dev);
            if (rc) return rc;
        }
        if (rs == FH_OK) {
            c->last_kernel = two_pass ? "k_assemble_vector_stream + k_vector_from_elements" : "k_assemble_vector_stream";
            return read_status(c, failed);
        }
        if (rs > 0) return rs;
        a.ke_out = nullptr;
    }
    c->last_kernel = "k_assemble_vector";
    a.epb = choose_epb(c, WHAT_VECTOR);
    a.ub = a.epb;
    const size_t lds = layout_bytes_dyn(c->elem_kind, c->op, WHAT_VECTOR, c->nq, a.ub, 0, 0, false);
    if (lds > LDS_LIMIT) return c->fail(FH_UNSUPPORTED, "quadrature rule too large for LDS staging");
    const int grid = (int)((a.work_end + a.epb - 1) / a.epb);
    rc = dispatch(all_kinds, c->elem_kind, elliptic_ops, c->op, (int)FH_OK, [&](auto ek, auto op) { return launch_vector<ek(), op()>(c, a, lds, grid); });
    if (rc) return rc;
    return read_status(c, failed);
}

int fh_assemble_vector(fh_ctx* c, double* out, uint64_t* failed) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int rc = check_ready(c, "fh_assemble_vector", false);
    if (rc) return rc;
    if (!out) return c->fail(FH_BAD_ARGUMENT, "fh_assemble_vector: out is null");
    return through_device(c, out, (size_t)c->S() * c->N, 0, true, [&](double* d) { return fh_assemble_vector_dev(c, d, failed); });
}

// ---- ElementSourceAssembler (src/assembly/local/source.rs) ------------------------------------------------------
extern "C++" int source_ready(fh_ctx* c, const char* who) {
    if (!c->has_mesh || c->ragged) return c->fail(FH_INVALID_STATE, std::string(who) + ": no finite element mesh set");
    if (c->nq <= 0) return c->fail(FH_INVALID_STATE, std::string(who) + ": no quadrature table set");
    return FH_OK;
}

int fh_assemble_source_vector_dev(fh_ctx* c, uint32_t sdim, const double* g, const double* values_dev, double* out_dev) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (c->rs.active) return c->fail(FH_UNSUPPORTED, "fh_assemble_source_vector: rule-set quadrature tables (fh_set_quadrature_rules) are not walked here");
    int rc = source_ready(c, "fh_assemble_source_vector");
    if (rc) return rc;
    const int D = c->ei.d;
    if (!out_dev) return c->fail(FH_BAD_ARGUMENT, "fh_assemble_source_vector: out is null");
    if (sdim != 1 && (int)sdim != D) return c->fail(FH_BAD_ARGUMENT, "fh_assemble_source_vector: solution dim must be 1 or the geometry dim");
    if (!values_dev && !g) return c->fail(FH_BAD_ARGUMENT, "fh_assemble_source_vector: neither g nor values given");
    if (!values_dev && !c->has_params)
        return c->fail(FH_INVALID_STATE, "fh_assemble_source_vector: the uniform source needs the density in the quadrature table");
    if (c->E == 0) return FH_OK;
    KArgs a = pass_args(c);
    SourceArgs sa{};
    sa.N = c->ei.n;
    sa.NG = c->ei.ng;
    sa.phigeom = c->phigeom.p;
    sa.values = values_dev;
    DevBuf<double> gd;      // device copy of g: only the one-pass scatter below reads it through a pointer
    SourceG gval{{0.0, 0.0, 0.0}};
    if (!values_dev)
        for (uint32_t k = 0; k < sdim; ++k) gval.v[k] = g[k];
    a.vec_out = out_dev;
    if (a.work_end == 0) return FH_OK;
    // small iso-parametric elements: the tiles of the residual (vector_tiles.hip) -- element vectors summed per distinct node of a tile
    // in LDS, partial sums through HBM, one thread per node; an element mask zeroes the inactive elements
    const bool fact = !values_dev;   // GravitySource: scalar partials / element entries, the node sum multiplies by g (element_pass.hpp)
    bool serve;
    rc = tile_partials(c, c->fe_scratch, fact ? 1 : (int)sdim, &serve);
    if (rc) return rc;
    if (serve && vector_tiles_source_pass(D, (int)sdim, c->ei.n, fact, c->stream, a, gval.v, sa.values, c->vt.v, active_mask(c), c->fe_scratch.p) == 0) {
        HIP_TRY(c, hipGetLastError());
        c->last_kernel = "k_source_elements_tiled + k_vector_from_partials";
        HIP_TRY(c, vector_tiles_node_pass(c->stream, (int)sdim, (int)c->N, c->vt.v, c->fe_scratch.p, out_dev, fact ? gval.v : nullptr));
        return FH_OK;
    }
    a.labels = active_labels(c);
    // two passes without atomics where the node adjacency is available (it comes with the pattern, which needs an operator
    // for the solution dimension): element vectors to scratch, then a per-row sum in element order
    bool two_pass = !a.labels && !c->ragged && c->op >= 0 && !c->opt.VECTOR_ATOMICS;
    if (two_pass && build_pattern(c) != FH_OK) two_pass = false;
    // a context without an operator (the usual case of a source assembler): the adjacency alone, for the element pass
    const unsigned *adj_off = nullptr, *adj = nullptr;
    if (!two_pass && !a.labels && c->op < 0 && element_pass_covers(c) && !c->opt.VECTOR_ATOMICS && build_source_adjacency(c) == FH_OK) {
        two_pass = true;
        adj_off = c->src_n2e_off.p;
        adj = c->src_n2e.p;
    }
    if (two_pass) {
        const size_t need = (size_t)c->E * c->ei.n * sdim;
        if (c->fe_scratch.n < need) HIP_TRY(c, c->fe_scratch.alloc(need));
        a.ke_out = c->fe_scratch.p;
    }
    if (two_pass && element_pass_covers(c)) {   // one thread per element, element vectors by local node, one thread per node (element_pass.hpp)
        const int ge = (int)((c->E + 255) / 256);
        double* fe = c->fe_scratch.p;
        dispatch(low_order_kinds, c->elem_kind, 0, [&](auto ek) {   // (element_pass_covers: one of these)
            constexpr int DV = ElemT<ek()>::D, NV = ElemT<ek()>::N;
            return dispatch_bool(sdim == 1, [&](auto scalar) {
                return dispatch_bool(fact, [&](auto fc) {
                    hipLaunchKernelGGL((k_source_elements<DV, scalar() ? 1 : DV, NV, fc()>), dim3(ge), dim3(256), 0, c->stream, a, gval, sa.values, fe);
                    return 0;
                });
            });
        });
        HIP_TRY(c, hipGetLastError());
        c->last_kernel = "k_source_elements + k_vector_from_elements_soa";
        return launch_vector_from_elements_soa(c, (int)sdim, fe, out_dev, adj_off, adj, fact ? &gval : nullptr);
    }
    if (adj_off) { two_pass = false; a.ke_out = nullptr; }   // (not covered after all: the one-pass scatter)
    if (!values_dev) {
        HIP_TRY(c, gd.alloc(sdim));
        HIP_TRY(c, hipMemcpyAsync(gd.p, g, sizeof(double) * sdim, hipMemcpyHostToDevice, c->stream));
        sa.g = gd.p;
    }
    a.epb = std::max(1, 256 / std::max(c->nq, c->ei.n));
    const size_t lds = sizeof(double) * (size_t)a.epb * c->nq;
    const int grid = (int)((a.work_end + a.epb - 1) / a.epb);
    c->last_kernel = "k_assemble_source";
    dispatch_or_last(int_list<2, 3>{}, D, [&](auto d) {
        return dispatch_bool(sdim == 1, [&](auto scalar) {
            hipLaunchKernelGGL((k_assemble_source<d(), scalar() ? 1 : d()>), dim3(grid), dim3(256), lds, c->stream, a, sa);
            return 0;
        });
    });
    HIP_TRY(c, hipGetLastError());
    if (two_pass) {
        rc = launch_vector_from_elements(c, (int)sdim, out_dev);
        if (rc) return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // gd is released on return
    return FH_OK;
}

int fh_assemble_source_vector(fh_ctx* c, uint32_t sdim, const double* g, const double* values, double* out) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int rc = source_ready(c, "fh_assemble_source_vector");
    if (rc) return rc;
    if (!out) return c->fail(FH_BAD_ARGUMENT, "fh_assemble_source_vector: out is null");
    const size_t nv = (size_t)c->E * c->nq * sdim;
    DevBuf<double> v;   // (input only; released after through_device's wait)
    return through_device(c, out, (size_t)sdim * c->N, 1, true, [&](double* d) {
        if (values) {
            HIP_TRY(c, v.alloc(nv + 1));
            HIP_TRY(c, hipMemcpyAsync(v.p, values, sizeof(double) * nv, hipMemcpyHostToDevice, c->stream));
        }
        return fh_assemble_source_vector_dev(c, sdim, g, values ? v.p : nullptr, d);
    });
}

int fh_physical_quadrature_points_dev(fh_ctx* c, double* x_dev) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (c->rs.active) return c->fail(FH_UNSUPPORTED, "fh_physical_quadrature_points: rule-set quadrature tables (fh_set_quadrature_rules) are not walked here");
    int rc = source_ready(c, "fh_physical_quadrature_points");
    if (rc) return rc;
    if (!x_dev) return c->fail(FH_BAD_ARGUMENT, "fh_physical_quadrature_points: output is null");
    if (c->E == 0) return FH_OK;
    KArgs a = pass_args(c);
    SourceArgs sa{};
    sa.N = c->ei.n;
    sa.NG = c->ei.ng;
    sa.phigeom = c->phigeom.p;
    sa.xq = x_dev;
    const long long total = (long long)c->E * c->nq;
    const int grid = (int)((total + 255) / 256);
    if (c->ei.d == 2) hipLaunchKernelGGL((k_physical_points<2>), dim3(grid), dim3(256), 0, c->stream, a, sa);
    else hipLaunchKernelGGL((k_physical_points<3>), dim3(grid), dim3(256), 0, c->stream, a, sa);
    HIP_TRY(c, hipGetLastError());
    return FH_OK;
}

int fh_physical_quadrature_points(fh_ctx* c, double* x) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int rc = source_ready(c, "fh_physical_quadrature_points");
    if (rc) return rc;
    if (!x) return c->fail(FH_BAD_ARGUMENT, "fh_physical_quadrature_points: output is null");
    return through_device(c, x, (size_t)c->E * c->nq * c->ei.d, 1, false, [&](double* d) { return fh_physical_quadrature_points_dev(c, d); });
}

static int assemble_scalar_single(fh_ctx* c, double* out, uint64_t* failed);
int fh_assemble_scalar(fh_ctx* c, double* out, uint64_t* failed) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (op_has_stress(c->op)) {
        const int rb = expansion_blocked(c, "fh_assemble_scalar");
        if (rb) return rb;
    }
    if (!c->rs.active) return assemble_scalar_single(c, out, failed);
    if (!out) return c->fail(FH_BAD_ARGUMENT, "fh_assemble_scalar: out is null");
    double tot = 0.0;
    const int rc = rs_walk_accumulating(c, failed, [&](uint64_t* f) {
        double part = 0.0;
        const int r = assemble_scalar_single(c, &part, f);
        tot += part;
        return r;
    });
    *out = tot;
    return rc;
}
static int assemble_scalar_single(fh_ctx* c, double* out, uint64_t* failed) {
    int rc = check_ready(c, "fh_assemble_scalar", false);
    if (rc) return rc;
    if (!op_has_stress(c->op)) return c->fail(FH_UNSUPPORTED, "fh_assemble_scalar: the mass assembler has no scalar form");
    if (!out) return c->fail(FH_BAD_ARGUMENT, "fh_assemble_scalar: out is null");
    rc = reset_status(c);
    if (rc) return rc;
    *out = 0.0;
    if (c->E == 0) return FH_OK;
    KArgs a = pass_args(c);
    if (a.work_end == 0) return FH_OK;
    // element tiles (vector_tiles.hip): the elements in the tiles' (space-compact) order -- what makes the gathers local on a numbering
    // without locality (C3's permuted tetrahedra: 0.76 -> 0.20 ms per call); an element mask zeroes the inactive elements' energies
    // (deliberately not tiles_enabled: the energy is a sum of partials whatever VECTOR_ATOMICS says, so that switch leaves it on the tiles;
    // one scalar per workgroup and their sum, not per-node partials: sized here)
    bool serve;
    rc = tile_partials(c, c->scalar_partial, 0, &serve, true);
    if (rc) return rc;
    if (serve) {
        const int grid = vector_tiles_energy_partials(c->vt.v);
        if (c->scalar_partial.n < (size_t)grid + 1) HIP_TRY(c, c->scalar_partial.alloc((size_t)grid + 1));
        if (vector_tiles_energy_pass(c->elem_kind, c->op, c->stream, a, c->vt.v, active_mask(c), c->scalar_partial.p) == grid) {
            HIP_TRY(c, hipGetLastError());
            c->last_kernel = "k_element_energy_tiled";
            hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, c->stream, c->scalar_partial.p, grid, c->scalar_partial.p + grid);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipMemcpyAsync(out, c->scalar_partial.p + grid, sizeof(double), hipMemcpyDeviceToHost, c->stream));
            return read_status(c, failed);
        }
    }
    a.labels = active_labels(c);
    if (!a.labels && element_pass_covers(c)) {
        // one thread per element (element_pass.hpp), workgroup partials in a fixed tree, the partials summed in index order by one
        // workgroup: one double comes back (global.rs:703-709 sums element by element; same terms, fixed association)
        const int grid = (int)((c->E + 255) / 256);
        DevBuf<double> partial;
        HIP_TRY(c, partial.alloc((size_t)grid + 1));
        a.scalar_out = partial.p;
        const int rs = launch_element_pass<EP_SCALAR>(c, a);
        if (rs == FH_OK) {
            c->last_kernel = "k_element_pass<scalar>";
            hipLaunchKernelGGL(k_sum_partials, dim3(1), dim3(256), 0, c->stream, partial.p, grid, partial.p + grid);
            HIP_TRY(c, hipGetLastError());
            HIP_TRY(c, hipMemcpyAsync(out, partial.p + grid, sizeof(double), hipMemcpyDeviceToHost, c->stream));
            return read_status(c, failed);
        }
        if (rs > 0) return rs;
    }
    // a batch of elements per workgroup: element energies summed in element order inside the batch, the batch partials in
    // order on the host (global.rs:703-709 sums element by element; same terms, fixed association)
    a.epb = std::max(1, std::min(choose_epb(c, WHAT_SCALAR), std::max(1, 256 / std::max(c->nq, 1))));
    a.ub = a.epb;
    const size_t lds = layout_bytes_dyn(c->elem_kind, c->op, WHAT_SCALAR, c->nq, a.ub, 0, 0, false);
    const int grid = (int)((a.work_end + a.epb - 1) / a.epb);
    DevBuf<double> partial;
    HIP_TRY(c, partial.alloc((size_t)grid));
    a.scalar_out = partial.p;
    c->last_kernel = "k_assemble_scalar";
    rc = dispatch(all_kinds, c->elem_kind, elliptic_ops, c->op, (int)FH_OK, [&](auto ek, auto op) { return launch_scalar<ek(), op()>(c, a, lds, grid); });
    if (rc) return rc;
    std::vector<double> h((size_t)grid);
    HIP_TRY(c, hipMemcpyAsync(h.data(), partial.p, sizeof(double) * grid, hipMemcpyDeviceToHost, c->stream));
    rc = read_status(c, failed);
    if (rc) return rc;
    double tot = 0.0;
    for (double v : h) tot += v;
    *out = tot;
    return FH_OK;
}

// ---- Dirichlet helpers
}  // extern "C"

// ---- the matrix-free map: y = T(u) x with T(u) = dr/du at the context's u (the matrix fh_assemble_matrix forms for the same context), and
// its diagonal, without a pattern or values.  For FH_LAPLACE and FH_LINEAR_ELASTIC the element vector is linear in u, so T(u) is the
// operator A of LinearOperator::apply (fenris-sparse/src/cg.rs:16-18) for every u, and the residual of the operand IS  A x:  the element pass
// of the residual, fed x in place of the context's u.  For FH_NEO_HOOKEAN, FH_STVK and FH_STABLE_NEO_HOOKEAN the element pass gathers u and the operand per
// element and forms dP(F)[grad x^T] per point (tangent_lin / tangent_apply, material.hpp).  On the tiles (Hex8, Tet4, Quad4, Tri3
// without a rule-set table) the node pass overwrites y, applies the Dirichlet rows on store and leaves the partials of x . y for CG;
// otherwise every group of a rule-set table takes the tiles where they cover it, else the per-element kernels, all accumulating into a
// zeroed y, and one more pass over y does the same.  Homogeneous Dirichlet nodes make the map the one fh_apply_dirichlet_csr_dev leaves
// (global.rs:379-451): the element pass reads x with their entries zeroed (their columns vanish), their rows are  scale x.
// LinearElastic: the element pass reads x 2^-e with |x 2^-e|_inf in [1/2, 1) (mf_exponent, device_common.hpp).
// scope: MF_OPERATOR for the operator's entry points (the operators linear in u), MF_TANGENT for the tangent's (every operator with a stress).
int mf_ready(fh_ctx* c, const char* who, int scope) {
    if (c->op == FH_LAPLACE || c->op == FH_TENSOR || c->rs.active) {   // (ahead of the other refusals: this one names the expansion)
        const int rb = expansion_blocked(c, who);
        if (rb) return rb;
    }
    if (c->op >= 0 && (!op_has_stress(c->op) || (scope == MF_OPERATOR && op_depends_on_u(c->op))))   // (no operator yet: check_ready says so)
        return c->fail(FH_UNSUPPORTED, std::string(who) + (scope == MF_OPERATOR
                                                               ? ": the matrix-free operator covers FH_LAPLACE and FH_LINEAR_ELASTIC only"
                                                               : ": the matrix-free tangent covers FH_LAPLACE, FH_LINEAR_ELASTIC, FH_NEO_HOOKEAN, FH_STVK and FH_STABLE_NEO_HOOKEAN"));
    const int rc = check_ready(c, who, false);
    if (rc) return rc;
    if (c->S() < 1 || c->S() > 3) return c->fail(FH_UNSUPPORTED, std::string(who) + ": solution dim must be 1..3");
    if (c->mf_num_dirichlet) {   // (late: the operator may have been set after the dofs)
        const int fit = dirichlet_components_fit(c, who, c->mf_comp_node, c->S());
        if (fit) return fit;
    }
    if (scope == MF_TANGENT) return contact_blocked(c, who);   // (the operator's entry points leave the contact term out)
    return FH_OK;
}

// what the scale of the Dirichlet rows depends on: mesh, vertices, operator, quadrature table and parameters, element mask (the setters of
// the last three move struct_gen), u for the nonlinear operators, and for the shifted map alpha M + beta T(u) its coefficients and (alpha != 0)
// the density, and the obstacles of fh_set_obstacles where the map includes them (their B(u) depends on u for every operator) -- not on
// which nodes are constrained.  The plain map is alpha = 0, beta = 1.
static void mf_scale_key_now(const fh_ctx* c, unsigned long long (&k)[8], double alpha = 0.0, double beta = 1.0) {
    const bool contact = contact_table(c).count != 0 && beta != 0.0;
    k[0] = c->struct_gen;
    k[1] = c->topo_gen;
    k[2] = c->geom_gen;
    // (the expansion joins u: both count upwards, so their sum moves when either does; 0 for the operators whose tangent does not see the field)
    k[3] = ((c->op <= FH_LINEAR_ELASTIC && !contact) || beta == 0.0) ? 0 : c->u_gen + expansion_key(c, true);
    std::memcpy(&k[4], &alpha, sizeof(double));
    std::memcpy(&k[5], &beta, sizeof(double));
    k[6] = alpha != 0.0 ? c->density_gen : 0;
    k[7] = contact ? contact_key(c) : 0;   // (contact_gen and friction_gen)
}

// the scale of the Dirichlet rows into c->mf_scale, from the unmodified diagonal (diag_dev) of alpha M + beta T(u)
static int mf_scale_from(fh_ctx* c, const double* diag_dev, double alpha = 0.0, double beta = 1.0) {
    const int n = c->S() * (int)c->N;
    DevBuf<unsigned long long> first;
    HIP_TRY(c, first.alloc(1));
    if (!c->mf_scale.p) HIP_TRY(c, c->mf_scale.alloc(1));
    HIP_TRY(c, hipMemsetAsync(first.p, 0xff, sizeof(unsigned long long), c->stream));
    if (n) hipLaunchKernelGGL(k_mf_first_nonzero, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, diag_dev, first.p);
    hipLaunchKernelGGL(k_mf_scale, dim3(1), dim3(64), 0, c->stream, diag_dev, first.p, c->mf_scale.p);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // (first is released on return)
    mf_scale_key_now(c, c->mf_scale_key, alpha, beta);
    return FH_OK;
}

// the element pass of the map over the tiles into c->fe_scratch (one partial per distinct node of a tile): the diagonal (xin null), the
// residual's element pass fed xin (linear operators), or k_tangent_tiled at the context's u.  *done = false: the tiles do not cover it.
static int mf_tiles_pass(fh_ctx* c, KArgs& a, const double* xin, bool* done) {
    *done = false;
    bool serve;
    const int rc = tile_partials(c, c->fe_scratch, c->S(), &serve);
    if (rc || !serve) return rc;
    const unsigned char* active = active_mask(c);
    int rt;
    if (!xin) {
        rt = vector_tiles_diagonal_pass(c->elem_kind, c->op, c->stream, a, c->vt.v, active, c->fe_scratch.p);
    } else if (c->op <= FH_LINEAR_ELASTIC) {
        a.u = xin;
        a.theta = nullptr;   // (the operand, not u: A x does not see the expansion)
        rt = vector_tiles_element_pass(c->elem_kind, c->op, c->stream, a, c->vt.v, active, c->fe_scratch.p);
    } else {
        rt = vector_tiles_tangent_pass(c->elem_kind, c->op, c->stream, a, c->vt.v, active, xin, c->fe_scratch.p);
    }
    if (rt != 0) return FH_OK;
    HIP_TRY(c, hipGetLastError());
    *done = true;
    return FH_OK;
}

// the per-element kernels of the map (solver_kernels.hpp) for the context's operator: the element diagonals (x null) or the element vectors
// of x into fe[a][e][c]
static void mf_elements_launch(fh_ctx* c, const KArgs& a, const unsigned char* active, const double* x, double* fe) {
    const dim3 grid((unsigned)((c->E + 255) / 256));
    dispatch_or_last(elliptic_ops, c->op, [&](auto op) {
        return dispatch_or_last(int_list<2, 3>{}, c->ei.d, [&](auto d) {
            constexpr int S = OpT<op(), d()>::S;
            // (the expansion: the nonlinear operators only -- the tangent of a linear one does not see it)
            return dispatch_bool(op_depends_on_u(op()) && a.theta != nullptr, [&](auto ex) {
                constexpr bool EX = ex() && op_depends_on_u(op());
                if (x) hipLaunchKernelGGL((k_mf_apply_elements<d(), S, op(), EX>), grid, dim3(256), 0, c->stream, a, c->ei.n, c->ei.ng, active, x, fe);
                else hipLaunchKernelGGL((k_mf_diagonal_elements<d(), S, op(), EX>), grid, dim3(256), 0, c->stream, a, c->ei.n, c->ei.ng, active, fe);
                return 0;
            });
        });
    });
}

// one quadrature table (or one group of a rule-set table): the element diagonals (xin null) or the element vectors of the operand xin ADDED
// to out -- the tiles where they cover it, else the per-element kernels and one thread per node over its (element, local node) entries in order
static int mf_single(fh_ctx* c, const double* xin, double* out, uint64_t* failed) {
    int rc = reset_status(c);
    if (rc) return rc;
    if (c->E == 0) return FH_OK;
    rc = ordered_single(
        c, out,
        [&](KArgs& a, bool* done) {
            const int r = mf_tiles_pass(c, a, xin, done);
            if (!r && *done)
                c->last_kernel = !xin                        ? "k_diagonal_tiled + k_vector_from_partials"
                                 : c->op <= FH_LINEAR_ELASTIC ? "k_element_pass_tiled + k_vector_from_partials"
                                                              : "k_tangent_tiled + k_vector_from_partials";
            return r;
        },
        [&](const KArgs& a, const unsigned char* active, double* fe) {
            mf_elements_launch(c, a, active, xin, fe);
            if (xin) c->last_kernel = "k_mf_apply_elements + k_vector_from_elements_soa";
            return (int)FH_OK;
        });
    return rc ? rc : read_status(c, failed);
}

// the operand of the map's element pass: x with the entries of the Dirichlet nodes zeroed and, for LinearElastic, scaled to |x 2^-e|_inf in
// [1/2, 1) over the free entries (mf_exponent; bits: the absolute maximum the node pass scales back by), in c->mf_xm; x itself where neither applies
struct MfOperand {
    const double* x;
    const unsigned long long* bits;
};
static int mf_operand(fh_ctx* c, const double* x, const unsigned char* dmask, MfOperand* in) {
    const int S = c->S(), n = S * (int)c->N;
    *in = MfOperand{x, nullptr};
    if (c->op == FH_LINEAR_ELASTIC) {
        if (!c->mf_bits.p) HIP_TRY(c, c->mf_bits.alloc(1));
        HIP_TRY(c, hipMemsetAsync(c->mf_bits.p, 0, sizeof(unsigned long long), c->stream));
        hipLaunchKernelGGL(k_mf_absmax, dim3(std::max(1, std::min(1024, (n + 255) / 256))), dim3(256), 0, c->stream, n, S, x, dmask, c->mf_bits.p);
        in->bits = c->mf_bits.p;
    }
    if (dmask || in->bits) {
        if (c->mf_xm.n < (size_t)n) HIP_TRY(c, c->mf_xm.alloc((size_t)n));
        hipLaunchKernelGGL(k_mf_operand, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, S, x, dmask, in->bits, c->mf_xm.p);
        HIP_TRY(c, hipGetLastError());
        in->x = c->mf_xm.p;
    }
    return FH_OK;
}

// T(u) x over every group of the table into out (S N doubles): the element sums alone -- every entry of x takes part, no Dirichlet rows, no
// contact term -- which is what the damping term eta_k T(u) v of the time integrators takes (the obstacle term stays out of C).  For the
// linear operators this is the residual's route run on the vector x (LinearElastic: on x 2^-e, scaled back).  Each group's status is reset
// and read.
int tangent_summed(fh_ctx* c, const double* x, double* out) {
    const int S = c->S(), n = S * (int)c->N;
    MfOperand in;
    int rc = mf_operand(c, x, nullptr, &in);
    if (rc) return rc;
    rc = walk_groups_into(c, out, (size_t)n, nullptr, [&](uint64_t* fl) { return mf_single(c, in.x, out, fl); });
    if (rc || !in.bits || !n) return rc;
    hipLaunchKernelGGL(k_mf_finish, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, S, x, (const unsigned char*)nullptr, (const double*)nullptr, in.bits,
                       out, (double*)nullptr);
    HIP_TRY(c, hipGetLastError());
    return FH_OK;
}

// where the g per-workgroup partials of x . y go: dot_scratch sized to them and *partials = g, or (dot_scratch null) nowhere
static int dot_partials(fh_ctx* c, DevBuf<double>* dot_scratch, int g, int* partials, double** dp) {
    *dp = nullptr;
    if (!dot_scratch) return FH_OK;
    if (dot_scratch->n < (size_t)g) HIP_TRY(c, dot_scratch->alloc((size_t)g));
    *dp = dot_scratch->p;
    *partials = g;
    return FH_OK;
}

// ---- the shifted map  y = (alpha M + beta T(u)) x: the mass M of the assembled FH_MASS_SCALAR / FH_MASS_VECTOR on the same mesh and table
// (I_s sum_q w |det J| rho phi_I phi_J, s the context operator's solution dim) with the density of fh_set_mass_density, and T(u) the map
// above.  The mass term is a pass of its own over the same tiles (k_mass_tiled; off the tiles k_mass_elements), after the tangent's kernels,
// which stay as they are; on the tiles one node pass sums the mass partials, adds beta T(u) x and writes the Dirichlet rows and the partials
// of x . y.  beta == 0 runs no stiffness work and does not read u; alpha == 0 runs the tangent alone.  Dirichlet nodes: the matrix
// fh_apply_dirichlet_csr_dev leaves of the assembled alpha M + beta K(u) (its scale from the shifted diagonal).
int mf_shift_ready(fh_ctx* c, const char* who, double alpha, double beta) {
    const int rc = mf_ready(c, who, MF_TANGENT);
    if (rc) return rc;
    if (!std::isfinite(alpha) || !std::isfinite(beta)) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": alpha and beta must be finite");
    if (alpha != 0.0 && c->mass_rho_n == 0) return c->fail(FH_INVALID_STATE, std::string(who) + ": alpha != 0 needs fh_set_mass_density");
    return FH_OK;
}

// the mass partials of the current table over the tiles into c->fe_scratch (x null: the diagonal); *done = false: the tiles do not cover it
static int mass_tiles_pass(fh_ctx* c, const KArgs& a, const double* x, const unsigned char* dmask, bool* done) {
    *done = false;
    if (c->ei.ng != c->ei.n) return FH_OK;
    bool serve;
    const int rc = tile_partials(c, c->fe_scratch, c->S(), &serve);
    if (rc || !serve) return rc;
    if (vector_tiles_mass_pass(c->elem_kind, c->S(), c->stream, a, c->vt.v, active_mask(c), c->mass_rho.p, c->mass_rho_n > 1 ? 1 : 0, x, dmask,
                               c->fe_scratch.p) != 0)
        return FH_OK;
    HIP_TRY(c, hipGetLastError());
    *done = true;
    return FH_OK;
}

// M x (x null: the diagonal of M) of the current table ADDED to out: the tiles where they cover it, else k_mass_elements and the ordered node sums
static int mass_single(fh_ctx* c, const double* x, const unsigned char* dmask, double* out) {
    if (c->E == 0 || (c->has_mask && c->num_active == 0)) return FH_OK;
    return ordered_single(
        c, out,
        [&](KArgs& a, bool* done) {
            const int r = mass_tiles_pass(c, a, x, dmask, done);
            if (!r && *done && !x) c->last_kernel = "k_mass_tiled + k_vector_from_partials";   // (the diagonal of M)
            return r;
        },
        [&](const KArgs& a, const unsigned char* active, double* fe) {
            const int covered = dispatch(all_kinds, c->elem_kind, -1, [&](auto ek) {
                using EL = ElemT<ek()>;
                return dispatch_bool(c->S() == 1, [&](auto scalar) {
                    hipLaunchKernelGGL((k_mass_elements<EL::D, scalar() ? 1 : EL::D, EL::N, EL::NG>), dim3((unsigned)((c->E + 255) / 256)), dim3(256), 0, c->stream,
                                       a, active, c->mass_rho.p, c->mass_rho_n > 1 ? 1 : 0, x, dmask, fe);
                    return 0;
                });
            });
            return covered < 0 ? c->fail(FH_UNSUPPORTED, "the shifted map: unknown element kind") : (int)FH_OK;
        });
}

// M x (x null: its diagonal) over every group of the table into out (S N doubles); the mass has no status to report
int mass_full(fh_ctx* c, const double* x, const unsigned char* dmask, double* out) {
    return walk_groups_into(c, out, (size_t)c->S() * c->N, nullptr, [&](uint64_t*) { return mass_single(c, x, dmask, out); });
}

// the diagonal of alpha M + beta T(u) into diag_dev (alpha = 0, beta = 1: of T(u) alone, nothing combined); with_scale: and, with Dirichlet
// nodes set, the scale of their rows (c->mf_scale) and their diagonal = scale
int mf_shift_diagonal(fh_ctx* c, double alpha, double beta, double* diag_dev, bool with_scale) {
    const bool plain = alpha == 0.0 && beta == 1.0;
    const int n = c->S() * (int)c->N;
    int rc;
    if (beta != 0.0) {
        uint64_t failed = 0;
        rc = walk_groups_into(c, diag_dev, (size_t)n, &failed, [&](uint64_t* f) { return mf_single(c, nullptr, diag_dev, f); });
        if (rc) return rc;
        rc = contact_add_diagonal(c, diag_dev);   // diag B(u) of the penalty contact term (k_contact_diagonal), before the scale is taken
        if (rc) return rc;
    }
    DevBuf<double> md;   // (once per solve: released on return, so that the solve holds no more than the apply)
    if (alpha != 0.0) {
        HIP_TRY(c, md.alloc((size_t)n + 1));
        rc = mass_full(c, nullptr, nullptr, md.p);
        if (rc) return rc;
    }
    if (!plain && n) {
        hipLaunchKernelGGL(k_mf_shift_combine, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, c->S(), alpha, alpha != 0.0 ? md.p : nullptr,
                           beta, beta != 0.0 ? diag_dev : nullptr, nullptr, nullptr, nullptr, diag_dev, nullptr);
        HIP_TRY(c, hipGetLastError());
    }
    if (c->mf_num_dirichlet && with_scale) {
        rc = mf_scale_from(c, diag_dev, alpha, beta);
        if (rc) return rc;
        hipLaunchKernelGGL(k_mf_dirichlet_diag, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, c->S(), c->mf_dmask.p, c->mf_scale.p, diag_dev);
        HIP_TRY(c, hipGetLastError());
    }
    if (md.p) HIP_TRY(c, hipStreamSynchronize(c->stream));   // (md is released on return)
    return FH_OK;
}

// the whole map in ONE element pass over the tiles, then the operator's node pass -- y overwritten, the Dirichlet rows, + beta B(u) x of the
// contact term, the partials of x . y.  The plain map (alpha = 0, beta = 1): the residual's element pass fed the operand, or k_tangent_tiled
// (mf_tiles_pass; `in`: the operand, prepared by the caller, who shares it with the route off the tiles).  alpha != 0: Hex8 with the monomial
// table only, the mass term fused into the element pass (vector_tiles_shifted_hex8_pass: beta T(u) x + alpha M x, or alpha M x alone for
// beta == 0, which reads x and dmask itself and needs no operand; M is linear, so the node pass scales LinearElastic's 2^-e back for both
// terms).  *done = false: not covered, nothing of the map was run.
static int map_on_tiles(fh_ctx* c, double alpha, double beta, const double* x, MfOperand in, double* y, DevBuf<double>* dot_scratch, int* partials,
                        bool* done) {
    *done = false;
    const int S = c->S(), N = (int)c->N;
    const unsigned char* dmask = c->mf_num_dirichlet ? c->mf_dmask.p : nullptr;
    const bool fused = alpha != 0.0, linear = c->op <= FH_LINEAR_ELASTIC;
    KArgs a = pass_args(c);
    int rc;
    if (fused) {
        if (c->elem_kind != FH_HEX8 || !a.qmono) return FH_OK;
        bool serve;
        rc = tile_partials(c, c->fe_scratch, S, &serve);
        if (rc || !serve) return rc;
        if (beta != 0.0) {
            rc = mf_operand(c, x, dmask, &in);
            if (rc) return rc;
            if (linear) {
                a.u = in.x;
                a.theta = nullptr;   // (the operand, not u)
            }
        }
        MassTerm mt;
        mt.alpha = alpha;
        mt.beta = beta;
        mt.rho = c->mass_rho.p;
        mt.per_elem = c->mass_rho_n > 1 ? 1 : 0;
        mt.mom = (a.all_affine && c->qmom_ok && c->qmom.p && !c->has_rules) ? c->qmom.p : nullptr;
        if (vector_tiles_shifted_hex8_pass(c->op, c->stream, a, c->vt.v, active_mask(c), in.x, dmask, mt, c->fe_scratch.p) != 0) return FH_OK;
        HIP_TRY(c, hipGetLastError());
    } else {
        bool passed;
        rc = mf_tiles_pass(c, a, in.x, &passed);
        if (rc || !passed) return rc;
    }
    double* dp;
    rc = dot_partials(c, dot_scratch, vector_tiles_operator_partials(N), partials, &dp);
    if (rc) return rc;
    c->last_kernel = !fused        ? (linear ? "k_element_pass_tiled + k_operator_from_partials" : "k_tangent_tiled + k_operator_from_partials")
                     : beta == 0.0 ? "k_mass_hex8_tiled + k_operator_from_partials"
                     : linear      ? "k_shifted_pass_tiled + k_operator_from_partials"
                                   : "k_shifted_tangent_tiled + k_operator_from_partials";
    HIP_TRY(c, vector_tiles_operator_node_pass(c->stream, S, N, c->vt.v, c->fe_scratch.p, x, dmask, c->mf_scale.p, in.bits, y, dp,
                                               beta != 0.0 ? contact_table(c) : contact_off(), beta));
    *done = true;
    return FH_OK;
}

// y = (alpha M + beta T(u)) x; alpha = 0, beta = 1: y = T(u) x.  The scale of the Dirichlet rows must be in c->mf_scale (mf_shift_diagonal).
// dot_scratch != null: per-workgroup partials of x . y go to it (*partials of them, in order).  Singular Jacobians land in the status slot: the
// caller resets and reads it.  The stages, each taken where it covers the call: the whole map on the tiles (map_on_tiles); the mass partials on
// the tiles and one node pass that adds beta T(u) x; everything composed -- T(u) x accumulated into y = 0 group by group, M x into scratch.
int mf_shift_apply(fh_ctx* c, double alpha, double beta, const double* x, double* y, DevBuf<double>* dot_scratch, int* partials) {
    const bool plain = alpha == 0.0 && beta == 1.0, one_table = c->E > 0 && !c->rs.active;
    const int S = c->S(), N = (int)c->N, n = S * N;
    const unsigned char* dmask = c->mf_num_dirichlet ? c->mf_dmask.p : nullptr;
    if (!plain && dmask && !c->mf_scale.p) HIP_TRY(c, c->mf_scale.alloc(1));
    int rc;
    bool done;
    double* dp;
    MfOperand in{x, nullptr};
    if (plain) {
        rc = mf_operand(c, x, dmask, &in);
        if (rc) return rc;
    }
    if (one_table && (plain || alpha != 0.0)) {
        rc = map_on_tiles(c, alpha, beta, x, in, y, dot_scratch, partials, &done);
        if (rc || done) return rc;
    }
    if (plain) {
        // elsewhere (kinds outside the tiles, rule-set groups, no tile tables): the element vectors of the operand accumulated into y = 0 without
        // atomics, group by group; then the scale, the Dirichlet rows and the partials of x . y
        uint64_t failed = 0;
        rc = walk_groups_into(c, y, (size_t)n, &failed, [&](uint64_t* f) { return mf_single(c, in.x, y, f); });
        if (rc) return rc;
        rc = contact_add_apply(c, x, dmask, in.bits, y);   // B(u) x of the penalty contact term (k_contact_apply), one launch, before the finish
        if (rc) return rc;
        const int g = (n + 255) / 256;
        rc = dot_partials(c, dot_scratch, g, partials, &dp);
        if (rc) return rc;
        if (dmask || dp || in.bits) {
            hipLaunchKernelGGL(k_mf_finish, dim3(g), dim3(256), 0, c->stream, n, S, x, dmask, c->mf_scale.p, in.bits, y, dp);
            HIP_TRY(c, hipGetLastError());
        }
        return FH_OK;
    }
    if (beta != 0.0) {   // T(u) x into y (its Dirichlet rows are written again below)
        rc = mf_shift_apply(c, 0.0, 1.0, x, y, nullptr, nullptr);
        if (rc) return rc;
    }
    if (alpha != 0.0 && one_table) {
        rc = mass_tiles_pass(c, pass_args(c), x, dmask, &done);
        if (rc) return rc;
        if (done) {
            rc = dot_partials(c, dot_scratch, vector_tiles_operator_partials(N), partials, &dp);
            if (rc) return rc;
            HIP_TRY(c, vector_tiles_shift_node_pass(c->stream, S, N, c->vt.v, c->fe_scratch.p, x, dmask, c->mf_scale.p, alpha, beta,
                                                    beta != 0.0 ? y : nullptr, y, dp));
            // (beta != 0: the name stays the one the tangent's pass above left, which the callers of the two-pass map know it by)
            if (beta == 0.0) c->last_kernel = "k_mass_tiled + k_shift_from_partials";
            return FH_OK;
        }
    }
    if (alpha != 0.0) {
        if (c->mf_mass.n < (size_t)n) HIP_TRY(c, c->mf_mass.alloc((size_t)n));
        rc = mass_full(c, x, dmask, c->mf_mass.p);
        if (rc) return rc;
    }
    const int g = (n + 255) / 256;
    rc = dot_partials(c, dot_scratch, g, partials, &dp);
    if (rc) return rc;
    if (n) {
        hipLaunchKernelGGL(k_mf_shift_combine, dim3(g), dim3(256), 0, c->stream, n, S, alpha, alpha != 0.0 ? c->mf_mass.p : nullptr, beta,
                           beta != 0.0 ? y : nullptr, x, dmask, c->mf_scale.p, y, dp);
        HIP_TRY(c, hipGetLastError());
    }
    return FH_OK;
}

// the entry points of the map and of its diagonal; alpha = 0, beta = 1 is the plain map of `scope`, every other pair the shifted tangent (scope
// MF_TANGENT, which is also the context's scope outside an entry point: the guard changes nothing for it).  The scale of the Dirichlet rows is
// formed again only when what it depends on has changed.
static int mf_apply_entry(fh_ctx* c, const char* who, int scope, double alpha, double beta, const double* x_dev, double* y_dev) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int rc = (alpha == 0.0 && beta == 1.0) ? mf_ready(c, who, scope) : mf_shift_ready(c, who, alpha, beta);
    if (rc) return rc;
    if (!x_dev || !y_dev) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null argument");
    if (c->N == 0) return FH_OK;
    MfScope scope_guard_(c, scope);
    unsigned long long key[8];
    mf_scale_key_now(c, key, alpha, beta);
    if (c->mf_num_dirichlet && !std::equal(key, key + 8, c->mf_scale_key)) {
        DevBuf<double> diag;
        HIP_TRY(c, diag.alloc((size_t)c->S() * c->N));
        rc = mf_shift_diagonal(c, alpha, beta, diag.p, true);
        if (rc) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    rc = reset_status(c);
    if (rc) return rc;
    rc = mf_shift_apply(c, alpha, beta, x_dev, y_dev, nullptr, nullptr);
    if (rc) return rc;
    return read_status(c, nullptr);
}

static int mf_diagonal_entry(fh_ctx* c, const char* who, int scope, double alpha, double beta, double* diag_dev) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int rc = (alpha == 0.0 && beta == 1.0) ? mf_ready(c, who, scope) : mf_shift_ready(c, who, alpha, beta);
    if (rc) return rc;
    if (!diag_dev) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null argument");
    if (c->N == 0) return FH_OK;
    MfScope scope_guard_(c, scope);
    rc = mf_shift_diagonal(c, alpha, beta, diag_dev, true);
    if (rc) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FH_OK;
}

// r(u) of the current table (or one group of a rule-set table) ADDED to out without atomics, on every element kind: k_residual_elements and
// the ordered node sums (the Newton residual off the tiles; fh_assemble_vector_dev scatters with fp64 atomics on the quadratic and cubic kinds)
static void residual_elements_launch(fh_ctx* c, const KArgs& a, const unsigned char* active, double* fe) {
    const dim3 grid((unsigned)((c->E + 255) / 256));
    dispatch_or_last(elliptic_ops, c->op, [&](auto op) {
        return dispatch_or_last(int_list<2, 3>{}, c->ei.d, [&](auto d) {
            return dispatch_bool(op_expands(op()) && a.theta != nullptr, [&](auto ex) {
                constexpr bool EX = ex() && op_expands(op());
                hipLaunchKernelGGL((k_residual_elements<d(), OpT<op(), d()>::S, op(), EX>), grid, dim3(256), 0, c->stream, a, c->ei.n, c->ei.ng, active, fe);
                return 0;
            });
        });
    });
}
static int residual_ordered_single(fh_ctx* c, double* out, uint64_t* failed) {
    int rc = reset_status(c);
    if (rc) return rc;
    if (c->E == 0 || (c->has_mask && c->num_active == 0)) return FH_OK;
    // (no tile launcher: newton_residual and the integrators own the tiles' branch, their node passes do more than sum)
    rc = ordered_single(c, out, nullptr, [&](const KArgs& a, const unsigned char* active, double* fe) {
        residual_elements_launch(c, a, active, fe);
        return (int)FH_OK;
    });
    return rc ? rc : read_status(c, failed);
}
// r(u) over every group of the table into out (S N doubles), and with obstacles set r + g (one launch of k_contact_force behind the node sums):
// what the Newton residual and the time integrators take off the tiles.  Each group's status is reset and read (a singular Jacobian is the
// error); no element is reported.
int residual_summed(fh_ctx* c, double* out) {
    const int rc = walk_groups_into(c, out, (size_t)c->S() * c->N, nullptr, [&](uint64_t* fl) { return residual_ordered_single(c, out, fl); });
    return rc ? rc : contact_add_force(c, out);
}

// ---- the Newton residual  F = alpha M (u - u_ref) + beta (r(u) - f)  at the context's u with the rows of the operator's Dirichlet nodes zero,
// and |F|^2 (fh_newton_solve_dev, engine_newton.hip).  On the tiles (Hex8, Tet4, Quad4, Tri3 without a rule-set table) the residual's element
// pass and, for alpha != 0, k_mass_tiled on d (all of it: the mass term of F sees the Dirichlet entries of d) leave their partials, and ONE
// node pass (k_newton_from_partials) forms F and the |F|^2 partials.  Elsewhere the residual (k_residual_elements and the ordered node sums,
// residual_summed) and M d (mass_full) land in scratch and k_newton_combine does the rest.  The partials are summed in a fixed order: bitwise
// reproducible.  Errors: those of the residual (FH_SINGULAR_JACOBIAN).  A point with det F <= 0 of NeoHookean makes F NaN, not an error.
int newton_residual(fh_ctx* c, double alpha, double beta, const double* f, const double* d, NewtonScratch& ns, double* norm2) {
    const int S = c->S(), N = (int)c->N, n = S * N;
    const unsigned char* dmask = c->mf_num_dirichlet ? c->mf_dmask.p : nullptr;
    int count = 0;   // per-workgroup partials of |F|^2 in ns.wg
    int rc;
    if (ns.F.n < (size_t)n) HIP_TRY(c, ns.F.alloc((size_t)n));
    bool serve = false;
    if (c->E > 0 && !c->rs.active && (alpha == 0.0 || c->ei.ng == c->ei.n)) {
        rc = tile_partials(c, ns.rpart, S, &serve);
        if (!rc && serve && alpha != 0.0) rc = tile_partials(c, ns.mpart, S, &serve);
        if (rc) return rc;
    }
    if (serve) {
        rc = reset_status(c);
        if (rc) return rc;
        const KArgs a = pass_args(c);
        const unsigned char* active = active_mask(c);
        bool ok = vector_tiles_element_pass(c->elem_kind, c->op, c->stream, a, c->vt.v, active, ns.rpart.p) == FH_OK;
        if (ok && alpha != 0.0)
            ok = vector_tiles_mass_pass(c->elem_kind, S, c->stream, a, c->vt.v, active, c->mass_rho.p, c->mass_rho_n > 1 ? 1 : 0, d, nullptr,
                                        ns.mpart.p) == 0;
        HIP_TRY(c, hipGetLastError());
        if (ok) {
            count = vector_tiles_operator_partials(N);
            if (ns.wg.n < (size_t)count) HIP_TRY(c, ns.wg.alloc((size_t)count));
            HIP_TRY(c, vector_tiles_newton_node_pass(c->stream, S, N, c->vt.v, ns.rpart.p, alpha != 0.0 ? ns.mpart.p : nullptr, f, dmask, alpha,
                                                     beta, ns.F.p, ns.wg.p, contact_table(c)));
            c->last_kernel = alpha != 0.0 ? "k_element_pass_tiled + k_mass_tiled + k_newton_from_partials"
                                          : "k_element_pass_tiled + k_newton_from_partials";
            rc = read_status(c, nullptr);
            if (rc) return rc;
        }
    }
    if (!count) {   // every other route: the residual and M d composed into scratch
        if (ns.r.n < (size_t)n) HIP_TRY(c, ns.r.alloc((size_t)n));
        rc = residual_summed(c, ns.r.p);
        if (rc) return rc;
        if (alpha != 0.0) {
            if (ns.m.n < (size_t)n) HIP_TRY(c, ns.m.alloc((size_t)n));
            rc = mass_full(c, d, nullptr, ns.m.p);
            if (rc) return rc;
        }
        count = std::max(1, (n + 255) / 256);
        if (ns.wg.n < (size_t)count) HIP_TRY(c, ns.wg.alloc((size_t)count));
        hipLaunchKernelGGL(k_newton_combine, dim3(count), dim3(256), 0, c->stream, n, S, alpha, alpha != 0.0 ? ns.m.p : nullptr, beta, ns.r.p, f,
                           dmask, ns.F.p, ns.wg.p);
        HIP_TRY(c, hipGetLastError());
        c->last_kernel = contact_table(c).count ? "k_residual_elements + k_vector_from_elements_soa + k_contact_force + k_newton_combine"
                                                : "k_residual_elements + k_vector_from_elements_soa + k_newton_combine";
    }
    const int ranges = std::min(2048, count);
    if (ns.sums.n < (size_t)ranges) HIP_TRY(c, ns.sums.alloc(2048));
    hipLaunchKernelGGL(k_sum_partial_ranges<1>, dim3(ranges), dim3(256), 0, c->stream, ns.wg.p, (long long)count, ns.sums.p);
    HIP_TRY(c, hipGetLastError());
    return sum_partials(c, ns.sums.p, ranges, 1, norm2);
}

extern "C" {

// the set of both entry points: components null = a node set, every component of each node
static int set_dirichlet(fh_ctx* c, const char* who, const uint64_t* nodes, const uint8_t* components, uint64_t num_nodes, bool by_dof) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (!c->has_mesh || c->ragged) return c->fail(FH_INVALID_STATE, std::string(who) + ": no finite element mesh set");
    if (num_nodes && !nodes) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null node list");
    if (by_dof && num_nodes && !components) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null component masks");
    if (!by_dof)
        for (uint64_t i = 0; i < num_nodes; ++i)
            if (nodes[i] >= c->N) return c->fail(FH_BAD_ARGUMENT, "Dirichlet node out of range");
    uint64_t comp_node[8];
    int rc = dirichlet_masks_to_device(c, who, nodes, components, num_nodes, nullptr, comp_node);   // (the checks, before anything is changed)
    if (rc) return rc;
    c->mf_num_dirichlet = 0;   // (the scale does not depend on which dofs are constrained: mf_scale stays valid)
    std::fill(c->mf_comp_node, c->mf_comp_node + 8, (uint64_t)0);
    ++c->dirichlet_gen;
    if (!nodes || num_nodes == 0) return FH_OK;
    const size_t bytes = ((size_t)c->N + 4) & ~(size_t)3;   // (whole words: k_mark_dofs)
    HIP_TRY(c, c->mf_dmask.alloc(bytes));
    HIP_TRY(c, hipMemsetAsync(c->mf_dmask.p, 0, bytes, c->stream));
    rc = dirichlet_masks_to_device(c, who, nodes, components, num_nodes, c->mf_dmask.p, comp_node);
    if (rc) return rc;
    std::copy(comp_node, comp_node + 8, c->mf_comp_node);
    c->mf_num_dirichlet = num_nodes;
    return FH_OK;
}

int fh_set_operator_dirichlet_nodes(fh_ctx* c, const uint64_t* nodes, uint64_t num_nodes) {
    return set_dirichlet(c, "fh_set_operator_dirichlet_nodes", nodes, nullptr, num_nodes, false);
}
int fh_set_operator_dirichlet_dofs(fh_ctx* c, const uint64_t* nodes, const uint8_t* components, uint64_t num_nodes) {
    return set_dirichlet(c, "fh_set_operator_dirichlet_dofs", nodes, components, num_nodes, true);
}

int fh_apply_operator_dev(fh_ctx* c, const double* x_dev, double* y_dev) {
    return mf_apply_entry(c, "fh_apply_operator_dev", MF_OPERATOR, 0.0, 1.0, x_dev, y_dev);
}
int fh_operator_diagonal_dev(fh_ctx* c, double* diag_dev) { return mf_diagonal_entry(c, "fh_operator_diagonal_dev", MF_OPERATOR, 0.0, 1.0, diag_dev); }
int fh_apply_tangent_dev(fh_ctx* c, const double* x_dev, double* y_dev) {
    return mf_apply_entry(c, "fh_apply_tangent_dev", MF_TANGENT, 0.0, 1.0, x_dev, y_dev);
}
int fh_tangent_diagonal_dev(fh_ctx* c, double* diag_dev) { return mf_diagonal_entry(c, "fh_tangent_diagonal_dev", MF_TANGENT, 0.0, 1.0, diag_dev); }

int fh_set_mass_density(fh_ctx* c, const double* rho, uint64_t count) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (!c->has_mesh || c->ragged) return c->fail(FH_INVALID_STATE, "fh_set_mass_density: no finite element mesh set");
    if (!rho) return c->fail(FH_BAD_ARGUMENT, "fh_set_mass_density: null density");
    if (count != 1 && count != c->E) return c->fail(FH_BAD_ARGUMENT, "fh_set_mass_density: count must be 1 or the number of elements");
    c->mass_rho_n = 0;
    HIP_TRY(c, c->mass_rho.alloc((size_t)count));
    HIP_TRY(c, hipMemcpyAsync(c->mass_rho.p, rho, sizeof(double) * count, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->mass_rho_n = count;
    ++c->density_gen;
    return FH_OK;
}

int fh_apply_shifted_tangent_dev(fh_ctx* c, double alpha, double beta, const double* x_dev, double* y_dev) {
    return mf_apply_entry(c, "fh_apply_shifted_tangent_dev", MF_TANGENT, alpha, beta, x_dev, y_dev);
}
int fh_shifted_tangent_diagonal_dev(fh_ctx* c, double alpha, double beta, double* diag_dev) {
    return mf_diagonal_entry(c, "fh_shifted_tangent_diagonal_dev", MF_TANGENT, alpha, beta, diag_dev);
}

}  // extern "C"
