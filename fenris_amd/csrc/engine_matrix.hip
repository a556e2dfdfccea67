// Stiffness / mass matrix launchers and their C ABI
#include "engine_internal.hpp"

template <int EK, int OP>
int launch_matrix(fh_ctx* c, KArgs& a, int mode, size_t lds_bytes, int grid) {
    if (grid <= 0) return FH_OK;   // nothing to do (an element mask without an active element): a launch of zero workgroups is an error
    const int rc = dispatch(int_list<MODE_ATOMIC, MODE_COLORED, MODE_GATHER, MODE_DUMP>{}, mode, -1, [&](auto m) {
        return launch_lds(c, k_assemble_matrix<EK, OP, m()>, dim3(grid), dim3(256), lds_bytes, c->stream, a);
    });
    return rc < 0 ? c->fail(FH_BAD_ARGUMENT, "bad scatter mode") : rc;
}

template <int EK, int OP>
size_t layout_bytes(int what, int nq, int ub, int acc, int nb, bool gather, int mb, int fast, int nc_row) {
    switch (what) {
        case WHAT_MATRIX: return make_layout<EK, OP, WHAT_MATRIX>(nq, ub, acc, nb, gather, mb, fast, 0, nc_row).bytes();
        case WHAT_VECTOR: return make_layout<EK, OP, WHAT_VECTOR>(nq, ub, acc, nb, gather, mb).bytes();
        default: return make_layout<EK, OP, WHAT_SCALAR>(nq, ub, acc, nb, gather, mb).bytes();
    }
}


size_t layout_bytes_dyn(int ek, int op, int what, int nq, int ub, int acc, int nb, bool gather, int mb, int fast, int nc_row) {
    return dispatch(all_kinds, ek, all_ops, op, (size_t)0,
                    [&](auto ekc, auto opc) { return layout_bytes<ekc(), opc()>(what, nq, ub, acc, nb, gather, mb, fast, nc_row); });
}


int choose_epb(fh_ctx* c, int what, size_t lds_target) {
    int best = 1;
    for (int epb = 1; epb <= 64; ++epb) {
        const size_t b = layout_bytes_dyn(c->elem_kind, c->op, what, c->nq, epb, 0, 0, false, 0, generic_fast(c));
        if (b <= lds_target) best = epb; else break;
    }
    return best;
}

// (an element kind or operator outside the lists: nothing is launched)
static int launch_matrix_dyn(fh_ctx* c, KArgs& a, int mode, size_t lds, int grid) {
    return dispatch(all_kinds, c->elem_kind, all_ops, c->op, (int)FH_OK,
                    [&](auto ek, auto op) { return launch_matrix<ek(), op()>(c, a, mode, lds, grid); });
}

template <int OP, bool ELEMPAR = false>
int launch_rows_tet4(fh_ctx* c, KArgs& a, const RowTablesS& T) {
    // the layout's integers + two parities of the record + the slot words
    const size_t lds = make_layout<FH_TET4, OP, WHAT_MATRIX>(a.nq, a.ub, 0, a.nb_max, true, 0, 1, 1, 0, 2).bytes() +
                       sizeof(int) * (size_t)(2 * T.rw + T.us + 4);
    if (lds > LDS_LIMIT) return c->fail(FH_UNSUPPORTED, "row-owner gather: LDS footprint too large");
    // workgroups per CU, measured inside one context on the same buffers (scripts/ab_in_context.py, C3): elasticity 2 (0.562 ms; 3: 0.594,
    // 4: 0.603, 5: 0.585), Laplace 4
    const size_t cap = (c->op == FH_LAPLACE) ? 4 : 2;
    const int per_cu = std::max(1, (int)std::min<size_t>(cap, (LDS_LIMIT - 512) / std::max<size_t>(lds, 1)));
    // (FENRIS_HIP_PIPE_GRID: tests force many positions per workgroup on small meshes)
    const int grid = std::max(1, std::min(c->npos_gen, c->opt.PIPE_GRID.value_or(c->num_cus * c->opt.PIPE_WGS_PER_CU.value_or(per_cu))));
    auto kern = a.trace ? k_gather_rows_tet4<OP, ELEMPAR, true> : k_gather_rows_tet4<OP, ELEMPAR>;   // FENRIS_HIP_TRACE: instrumented twin
    if (c->opt.VERBOSE)
        std::fprintf(stderr, "[fenris_hip] row-owner gather (Tet4): lds=%zu B wgs/cu=%d grid=%d\n", lds, per_cu, grid);
    return launch_lds(c, kern, dim3(grid), dim3(256), lds, c->stream, a, T);
}

template <int EK, int OP, int QC, int JT>
int launch_pipelined_j(fh_ctx* c, KArgs& a, const PipeTables& T) {
    size_t lds = make_layout<EK, OP, WHAT_MATRIX>(a.nq, a.ub, a.acc_max, a.nb_max, true, a.mb, 1, QC).bytes();
    if (lds > LDS_LIMIT) return c->fail(FH_UNSUPPORTED, "pipelined gather: LDS footprint too large");
    // the compile-time-rule instantiation (Hex8, rule of exactly QC points) stages planar gradient rows, which are
    // longer: taken only while two workgroups still share a CU
    bool fullq = false;
    if constexpr (EK == FH_HEX8 && QC == 8 && JT == 2) {
        const size_t lds_planar = make_layout<EK, OP, WHAT_MATRIX>(a.nq, a.ub, a.acc_max, a.nb_max, true, a.mb, 1, QC, 0, 1).bytes();
        fullq = a.nq == QC && T.cs <= 256 && T.rw <= 256 &&
                (2 * lds_planar + 1024 <= LDS_LIMIT || 2 * lds + 1024 > LDS_LIMIT);
        if (fullq) lds = lds_planar;
    }
    const int per_cu = std::max(1, (int)std::min<size_t>(8, (LDS_LIMIT - 512) / std::max<size_t>(lds, 1)));
    const int wgs = std::max(1, c->opt.PIPE_WGS_PER_CU.value_or(per_cu));
    const int grid = std::max(1, std::min(c->npos_gen, c->opt.PIPE_GRID.value_or(c->num_cus * wgs)));
    // the instrumented instantiation only where it is used for profiling (Hex8, the default tiling)
    const bool dbg = (c->opt.TRACE || c->opt.ABLATE.set);
    void (*kern)(const KArgs, const PipeTables) = k_gather_pipelined<EK, OP, QC, JT>;
    constexpr int N_ = ElemT<EK>::N;
    constexpr bool DEFAULT_JT = JT == ((N_ % 2 == 0) ? 2 : N_);  // per-element data: the default tiling only
    if (T.slotpar) {
        if constexpr (OP == FH_LINEAR_ELASTIC && DEFAULT_JT) {
            kern = k_gather_pipelined<EK, OP, QC, JT, false, false, true>;
            if constexpr (EK == FH_HEX8 && QC == 8 && JT == 2)
                if (fullq) kern = k_gather_pipelined<EK, OP, QC, JT, false, true, true>;
        } else {
            return c->fail(FH_UNSUPPORTED, "pipelined gather with per-element parameters: default FENRIS_HIP_PIPE_JT only");
        }
    } else if constexpr (EK == FH_TET4 && QC == 1 && JT == 2) {
        if (dbg) kern = k_gather_pipelined<EK, OP, QC, JT, true>;
    } else if constexpr (EK == FH_HEX8 && QC == 8 && JT == 2) {
        if (dbg) {  // the instrumented twin of whichever instantiation production would take
            if (fullq) kern = k_gather_pipelined<EK, OP, QC, JT, true, true>;
            else kern = k_gather_pipelined<EK, OP, QC, JT, true>;
        } else if (fullq)
            kern = k_gather_pipelined<EK, OP, QC, JT, false, true>;
    }
    if (c->opt.VERBOSE)
        std::fprintf(stderr, "[fenris_hip] pipelined gather: QC=%d JT=%d lds=%zu B wgs/cu=%d grid=%d\n", QC, JT, lds, wgs, grid);
    return launch_lds(c, kern, dim3(grid), dim3(256), lds, c->stream, a, T);
}

template <int EK, int OP, int QC>
int launch_pipelined_q(fh_ctx* c, KArgs& a, const PipeTables& T) {
    constexpr int N = ElemT<EK>::N;
    const int jt = c->p_jt;
    if (N % 4 == 0 && jt == 4) return launch_pipelined_j<EK, OP, QC, 4>(c, a, T);
    if (N % 2 == 0 && jt == 2) return launch_pipelined_j<EK, OP, QC, 2>(c, a, T);
    if (jt == N) return launch_pipelined_j<EK, OP, QC, N>(c, a, T);
    return launch_pipelined_j<EK, OP, QC, 1>(c, a, T);
}

template <int EK, int OP>
int launch_pipelined_t(fh_ctx* c, KArgs& a, const PipeTables& T, size_t, int) {
    // staged quadrature points per chunk: the largest chunk (not larger than the rule) that still lets >= 2
    // workgroups share a CU (measured on Hex8: profiles/r01_sweep_128_pipelined_nb_qc_jt.txt)
    int qc = c->opt.PIPE_QC.value_or(0);
    if (qc <= 0) {
        qc = 1;
        for (int cand : {8, 4, 2}) {
            if (cand > a.nq && cand > 1 && cand / 2 >= a.nq) continue;  // would stage empty slots
            const size_t lds = make_layout<EK, OP, WHAT_MATRIX>(a.nq, a.ub, a.acc_max, a.nb_max, true, a.mb, 1, cand).bytes();
            if (2 * lds + 1024 <= LDS_LIMIT) { qc = cand; break; }
        }
    }
    if (a.nq == 1) qc = 1;
    if (qc >= 8) return launch_pipelined_q<EK, OP, 8>(c, a, T);
    if (qc >= 4) return launch_pipelined_q<EK, OP, 4>(c, a, T);
    if (qc >= 2) return launch_pipelined_q<EK, OP, 2>(c, a, T);
    return launch_pipelined_q<EK, OP, 1>(c, a, T);
}

int launch_pipelined(fh_ctx* c, KArgs& a, const PipeTables& T, size_t lds, int grid) {
    const bool lap = c->op == FH_LAPLACE;
    switch (c->elem_kind) {
        case FH_HEX8: return lap ? launch_pipelined_t<FH_HEX8, FH_LAPLACE>(c, a, T, lds, grid)
                                 : launch_pipelined_t<FH_HEX8, FH_LINEAR_ELASTIC>(c, a, T, lds, grid);
        case FH_TET4: return lap ? launch_pipelined_t<FH_TET4, FH_LAPLACE>(c, a, T, lds, grid)
                                 : launch_pipelined_t<FH_TET4, FH_LINEAR_ELASTIC>(c, a, T, lds, grid);
        case FH_QUAD4: return lap ? launch_pipelined_t<FH_QUAD4, FH_LAPLACE>(c, a, T, lds, grid)
                                  : launch_pipelined_t<FH_QUAD4, FH_LINEAR_ELASTIC>(c, a, T, lds, grid);
        case FH_TRI3: return lap ? launch_pipelined_t<FH_TRI3, FH_LAPLACE>(c, a, T, lds, grid)
                                 : launch_pipelined_t<FH_TRI3, FH_LINEAR_ELASTIC>(c, a, T, lds, grid);
        default: return c->fail(FH_UNSUPPORTED, "pipelined gather: unsupported element");
    }
}

// Shared records and slot lists of the affine sweep (fh_ctx::a_shared): on a structured, graded or extruded mesh most affine elements have
// bit-identical records, and most positions the same list of them.  Two 64-bit hashes per record (per list) from the device, merged here on
// equality of the 128 bits like the lane tables (build_lane_tables), then a pass in which every element (position) compares itself bit for
// bit with the table entry it was given: the sweep then reads a few hundred KB that stay in the caches instead of E records and npos lists
// beside its own row stores.  Equality is of BITS: congruent elements whose coordinates round differently keep records of their own.
// Runs behind the records pass when its key moved; costs three round trips and one pass over the records, once per mesh generation.
static int affine_shared_prepare(fh_ctx* c, int gw, long long e_lo, long long e_hi, bool dbg, bool& use) {
    auto& sh = c->a_shared;
    use = false;
    auto off = [&](const char* why) { sh.on = false; sh.nrec = sh.nvec = 0; sh.reason = sh.build_reason = why; return (int)FH_OK; };
    // states that need no tables (and leave the ones there are alone)
    // Elasticity by default.  The Laplace / mass sweep is bound by the scalar unit and LDS, not by memory (profiles/r06_c2_lds_bound.txt), and its
    // loader's extra level of indirection costs more than the reads it saves: 0.296 against 0.205 ms on 128^3 Poisson in one context
    // (profiles/affine_shared_records.txt item 8).  The form is there and exact; FENRIS_HIP_AFFINE_SHARED=1 selects it.
    if (!c->opt.AFFINE_SHARED.value_or(gw == AFFINE_ROWS_GW_LE ? 1 : 0)) {
        sh.reason = c->opt.AFFINE_SHARED.set ? "switched off (FENRIS_HIP_AFFINE_SHARED=0)"
                                             : "Laplace / mass: per-element loader unless FENRIS_HIP_AFFINE_SHARED=1";
        return FH_OK;
    }
    if (c->has_mask) { sh.reason = "element mask: per-element loader"; return FH_OK; }
    if (c->row_hi >= 0 || c->status_slot != 0) { sh.reason = "row range: per-element loader"; return FH_OK; }
    if (dbg) { sh.reason = "instrumented launch: per-element loader"; return FH_OK; }
    const int max_rec = std::min(c->opt.AFFINE_SHARED_MAX_RECORDS.value_or(4096), 0xfffe);
    const int max_vec = std::min(c->opt.AFFINE_SHARED_MAX_LISTS.value_or(8192), 1 << 22);
    const bool same_key = sh.gen == c->a_geom_gen && sh.op == c->op && sh.lo == e_lo && sh.hi == e_hi && sh.struct_gen == c->struct_gen &&
                          sh.hdr == (const void*)c->a_hdr.p && sh.npos == c->a_npos && sh.max_rec == max_rec && sh.max_vec == max_vec;
    if (sh.built && same_key) {   // current
        sh.reason = sh.on ? "" : sh.build_reason;
        use = sh.on;
        return FH_OK;
    }
    if (!same_key) {
        sh.gen = c->a_geom_gen; sh.op = c->op; sh.lo = e_lo; sh.hi = e_hi; sh.struct_gen = c->struct_gen; sh.hdr = c->a_hdr.p; sh.npos = c->a_npos;
        sh.max_rec = max_rec; sh.max_vec = max_vec;
        sh.built = false; sh.seen = 0;
        off("");
    }
    {   // not for a generation that may be gone after one assembly (fh_ctx::a_shared)
        const long long need = (long long)std::max(0, c->opt.AFFINE_SHARED_AFTER.value_or(2)) << std::min(sh.fails, 20);
        if (!c->a_shared_now && sh.seen < need) {
            ++sh.seen;
            sh.reason = "tables not built yet: the first sweeps of a mesh generation keep the per-element loader";
            return FH_OK;
        }
    }
    sh.built = true;
    const auto t_build = std::chrono::steady_clock::now();
    struct BuildTime {   // every way out of the build
        decltype(c->a_shared)& s; std::chrono::steady_clock::time_point t0; bool verbose;
        ~BuildTime() {
            s.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            const bool over = !s.on && std::strstr(s.build_reason, "limit") != nullptr;
            s.fails = over ? std::min(s.fails + 1, 20) : 0;
            if (verbose) std::fprintf(stderr, "[fenris_hip] affine rows, shared form: table build took %.1f ms (%s)\n", s.build_ms, s.on ? "shared" : s.build_reason);
        }
    } build_time{sh, t_build, c->opt.VERBOSE};
    const long long n = e_hi - e_lo;
    const int npos = c->a_npos, us = c->a_us;
    if (n <= 0 || npos <= 0) return off("no affine positions");
    // 1. distinct records
    DevBuf<unsigned long long> hash_d;
    HIP_TRY(c, hash_d.alloc((size_t)2 * std::max<long long>(n, npos)));
    HostBuf<unsigned long long> hash_h((size_t)2 * std::max<long long>(n, npos));
    HIP_TRY(c, affine_shared_hash_records(gw, c->stream, c->a_recs.p, c->elem_aff.p, e_lo, e_hi, hash_d.p));
    HIP_TRY(c, hipMemcpyAsync(hash_h.data(), hash_d.p, sizeof(unsigned long long) * (size_t)n * 2, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HostBuf<unsigned short> cls_h((size_t)n);
    hvec<long long> first;
    {
        std::unordered_map<unsigned long long, int> seen;
        seen.reserve(1024);
        unsigned long long p1 = 0ull, p2 = 0ull;   // the element before: neighbours mostly agree
        int pc = 0xffff;
        for (long long i = 0; i < n; ++i) {
            const unsigned long long h1 = hash_h[(size_t)i], h2 = hash_h[(size_t)(n + i)];
            if (h1 == p1 && h2 == p2) { cls_h[(size_t)i] = (unsigned short)pc; continue; }
            p1 = h1; p2 = h2;
            if (!h1 && !h2) { pc = 0xffff; cls_h[(size_t)i] = 0xffff; continue; }   // not affine
            auto it = seen.find(h1);
            if (it == seen.end()) {
                if ((int)first.size() >= max_rec) return off("more distinct records than the limit");
                it = seen.emplace(h1, (int)first.size()).first;
                first.push_back(e_lo + i);
            } else if (hash_h[(size_t)(n + first[(size_t)it->second] - e_lo)] != h2) {
                return off("hash collision among the records");
            }
            pc = it->second;
            cls_h[(size_t)i] = (unsigned short)pc;
        }
    }
    const int nrec = (int)first.size();
    if (nrec == 0) return off("no affine elements");
    DevBuf<long long> first_d;
    DevBuf<int> st;
    HIP_TRY(c, first_d.alloc((size_t)nrec));
    HIP_TRY(c, st.alloc(2));
    HIP_TRY(c, hipMemsetAsync(st.p, 0, 2 * sizeof(int), c->stream));
    if (c->a_cls.n < (size_t)c->E) HIP_TRY(c, c->a_cls.alloc((size_t)c->E));
    HIP_TRY(c, c->a_rec_tab.alloc((size_t)nrec * gw));
    HIP_TRY(c, hipMemcpyAsync(c->a_cls.p + e_lo, cls_h.data(), sizeof(unsigned short) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(first_d.p, first.data(), sizeof(long long) * (size_t)nrec, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, affine_shared_record_table(gw, c->stream, c->a_recs.p, c->elem_aff.p, c->a_cls.p, first_d.p, nrec, e_lo, e_hi, c->a_rec_tab.p, st.p));
    // 2. distinct lists of slot classes
    HIP_TRY(c, affine_shared_hash_lists(c->stream, c->a_elem.p, c->a_cls.p, npos, us, hash_d.p));
    int mismatch[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(mismatch, st.p, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(hash_h.data(), hash_d.p, sizeof(unsigned long long) * (size_t)npos * 2, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (mismatch[0]) return off("an element's record differs from its table entry");
    HostBuf<int> ids((size_t)npos);
    hvec<int> first_pos;
    {
        std::unordered_map<unsigned long long, int> seen;
        seen.reserve(1024);
        for (int p = 0; p < npos; ++p) {
            const unsigned long long h1 = hash_h[(size_t)p], h2 = hash_h[(size_t)npos + p];
            auto it = seen.find(h1);
            if (it == seen.end()) {
                if ((int)first_pos.size() >= max_vec) return off("more distinct slot lists than the limit");
                it = seen.emplace(h1, (int)first_pos.size()).first;
                first_pos.push_back(p);
            } else if (hash_h[(size_t)npos + first_pos[(size_t)it->second]] != h2) {
                return off("hash collision among the slot lists");
            }
            ids[(size_t)p] = it->second;
        }
    }
    const int nvec = (int)first_pos.size();
    DevBuf<int> ids_d, first_pos_d;
    HIP_TRY(c, ids_d.alloc((size_t)npos));
    HIP_TRY(c, first_pos_d.alloc((size_t)nvec));
    HIP_TRY(c, c->a_slot_tab.alloc((size_t)nvec * us));
    HIP_TRY(c, hipMemcpyAsync(ids_d.p, ids.data(), sizeof(int) * (size_t)npos, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(first_pos_d.p, first_pos.data(), sizeof(int) * (size_t)nvec, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, affine_shared_list_table(c->stream, c->a_elem.p, c->a_cls.p, ids_d.p, first_pos_d.p, npos, nvec, us, c->a_slot_tab.p, c->a_hdr.p, st.p + 1));
    HIP_TRY(c, hipMemcpyAsync(mismatch, st.p, 2 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (mismatch[1]) return off("a position's slot list differs from its table entry");
    sh.on = true; sh.nrec = nrec; sh.nvec = nvec; sh.reason = sh.build_reason = "";
    use = true;
    if (c->opt.VERBOSE)
        std::fprintf(stderr, "[fenris_hip] affine rows, shared form: %lld elements share %d records, %d positions share %d slot lists\n", n, nrec, npos, nvec);
    return FH_OK;
}

// node blocks all of whose elements are affine: k_affine_rows (affine_rows.hip) over their position tables, behind k_affine_records where
// the element records are not current
int launch_affine(fh_ctx* c, KArgs& a) {
    // the scalar mass matrix rides the Laplace kernel: records (|det J|, 0 ...), reference blocks (sum_q w rho phi_a phi_b, 0 ...)
    const int rop = (c->op == FH_MASS_SCALAR) ? (int)FH_LAPLACE : c->op;
    const int gw = (rop == FH_LAPLACE) ? AFFINE_ROWS_GW_LAP : AFFINE_ROWS_GW_LE;
    // (Measured and retired to scripts/attic/: the element records formed inside k_affine_rows by a seventh wavefront -- 4.82 against 4.73 ms on the
    // headline, profiles/r05_fused_records_experiment.txt; the barrier-free ring form, affine_ring.hip -- 5 % slower; positions dealt in chunks
    // instead of one contiguous range per workgroup, profiles/r04_chunk_experiment.txt; non-temporal row stores for elasticity; two store waves.)
    const int a_depth = c->opt.AFFINE_DEPTH.value_or(2);
    if (c->a_recs.n < (size_t)c->E * gw) { HIP_TRY(c, c->a_recs.alloc((size_t)c->E * gw)); ++c->a_recs_gen; }
    if (c->a_sing.n < affine_sing_words(c->E)) { HIP_TRY(c, c->a_sing.alloc(affine_sing_words(c->E))); ++c->a_recs_gen; }
    const unsigned char* act = c->has_mask ? c->active.p : nullptr;
    DevStatus* status = c->status.p + c->status_slot;
    const int nt = (rop == FH_LAPLACE ? AFFINE_ROWS_NT_STORES : 0) | ((c->opt.AFFINE_PRIO.value_or(3 | (2 << 2)) & 15) << AFFINE_ROWS_PRIO_SHIFT);
    bool shared = false;
    auto rows = [&](int pos0, int count) -> int {
        AffineRowTables T{c->a_hdr.p, c->a_lanes.p, {c->a_elem.p}, {c->a_recs.p},
                          c->ghat.p + (c->op == FH_MASS_SCALAR ? 64 * (AFFINE_GW_LE + AFFINE_GW_LAP) : c->op == FH_LAPLACE ? 64 * AFFINE_GW_LE : 0), c->a_us, count,
                          c->g_acc, pos0, c->a_npos, c->a_incomplete};
        const size_t lds = affine_rows_lds_bytes(rop, c->a_us, c->g_acc);
        if (lds > LDS_LIMIT) return c->fail(FH_UNSUPPORTED, "affine gather: LDS footprint too large");
        // workgroups per CU, measured best: 3 (elasticity), 4 (Laplace: fewer registers, less LDS)
        const int per_cu = std::max(1, (int)std::min<size_t>(rop == FH_LAPLACE ? 4 : 3, (LDS_LIMIT - 512) / std::max<size_t>(lds, 1)));
        const int grid = std::max(1, std::min(count, c->opt.AFFINE_GRID.value_or(c->num_cus * c->opt.AFFINE_WGS_PER_CU.value_or(per_cu))));
        if (c->opt.VERBOSE)
            std::fprintf(stderr, "[fenris_hip] affine rows: positions %d + %d lds=%zu B wgs/cu=%d grid=%d\n", pos0, count, lds, per_cu, grid);
        if (shared) { T.slot_tab = c->a_slot_tab.p; T.rec_tab = c->a_rec_tab.p; }
        HIP_TRY(c, affine_rows_launch(rop, a_depth, grid, lds, c->stream, a, T, a.ablate | nt, c->has_mask, shared));
        return FH_OK;
    };
    // Element records (R = sqrt|det J| J^-1 or M = R R^T per affine element) on the same stream in front of the sweep -- but only those that are
    // not current (fh_ctx::a_recs_valid): they are a function of the context's vertices, connectivity and affine flags, not of the material,
    // the flags of the call or the values, so a caller that assembles again on an unchanged mesh (time steps, material sweeps, the interface and
    // main launches of a slab step) gets ONE launch per assembly.  The sweep reads them from memory either way: 20 GB of rows are written
    // between their production and their use.  FENRIS_HIP_AFFINE_RECORDS_ALWAYS=1 runs the pass in every assembly, as before.
    // (Round 3: making the records of all but the first eighth of the sweep on a second stream beside the first part's launch was measured
    // 0.3 ms SLOWER than the 0.41 ms it hides -- the two kernels' workgroups compete for the CUs; two launches of the sweep in one stream cost
    // nothing measurable, and records made chunk by chunk right before their part of the sweep (to be read back from the memory-side
    // cache) change nothing up to 4 chunks and lose from 8 on.  profiles/r03_affine_experiments.txt)
    const long long e_lo = c->a_emin, e_hi = std::min<long long>(c->a_emax + 1, (long long)c->E);
    auto& v = c->a_recs_valid;
    const bool current = v.gen == c->a_recs_gen && v.op == c->op;
    const bool covered = current && v.lo <= e_lo && e_hi <= v.hi;
    if (!covered || c->opt.AFFINE_RECORDS_ALWAYS.value_or(0)) {
        // the marks of singular elements belong to one generation and format: cleared when either moves
        if (!current) HIP_TRY(c, hipMemsetAsync(c->a_sing.p, 0, sizeof(unsigned) * c->a_sing.n, c->stream));
        if (c->opt.VERBOSE)
            std::fprintf(stderr, "[fenris_hip] affine records computed: elements [%lld, %lld)\n", e_lo, e_hi);
        HIP_TRY(c, affine_records_launch(c->op, c->stream, c->verts.p, c->conn.p, c->elem_aff.p, act, e_lo, e_hi, c->a_recs.p, status, c->a_sing.p));
        if (current && e_lo <= v.hi && v.lo <= e_hi) {   // touches or overlaps what is valid: the union
            v.lo = std::min(v.lo, e_lo);
            v.hi = std::max(v.hi, e_hi);
        } else {
            v.lo = e_lo; v.hi = e_hi; v.op = c->op; v.gen = c->a_recs_gen;
        }
    } else {
        // the records pass is also what reports a singular affine element: its marks repeat the report, for this range and this mask
        HIP_TRY(c, affine_replay_singular_launch(c->stream, c->a_sing.p, act, e_lo, e_hi, status));
    }
    const int rc_shared = affine_shared_prepare(c, gw, e_lo, e_hi, (a.ablate & 0xffff) != 0, shared);
    if (rc_shared) return rc_shared;
    c->a_shared.used = shared;
    return rows(0, c->a_npos);
}

// dense element matrices of the elements [first, first + count) into device memory (no status read-back)
int element_matrices_enqueue(fh_ctx* c, uint64_t first, uint64_t count, double* ke_dev, bool by_elem, bool tri) {
    KArgs a;
    fill_common(c, a);
    a.ke_out = ke_dev;
    a.ke_by_elem = by_elem ? 1 : 0;
    a.ke_tri = tri ? 1 : 0;
    if (by_elem && (a.nonsym & 1)) a.nonsym |= 2;   // two-pass assembly of a non-symmetric operator: K_e transposed (the gather reads columns as rows)
    a.labels = (by_elem && c->has_mask) ? c->active_list.p : nullptr;  // two-pass assembly: the active elements only
    a.work_begin = (long long)first;
    a.work_end = (long long)(first + count);
    // elements per workgroup by an LDS budget of 52 KB = THREE workgroups per CU (the other generic kernels: 64 KB, two): Hex8 NeoHookean 128^3 6.24 -> 5.66 ms,
    // StVK 7.31 -> 6.64, Tet10 / Tet4 level; 39 KB (four) is level or worse (profiles/r06_two_pass_triangles_generic.txt)
    a.epb = choose_epb(c, WHAT_MATRIX, (size_t)52 * 1024);
    a.ub = a.epb;
    const size_t lds = layout_bytes_dyn(c->elem_kind, c->op, WHAT_MATRIX, c->nq, a.ub, 0, 0, false, 0, a.fast);
    if (lds > LDS_LIMIT) return c->fail(FH_UNSUPPORTED, "quadrature rule too large for LDS staging");
    const int grid = (int)((count + a.epb - 1) / a.epb);
    return launch_matrix_dyn(c, a, MODE_DUMP, lds, grid);
}

// Which kernel the general positions (those not in the affine class) of an FH_SCATTER_GATHER assembly run on: ONE rule, read by the dispatch below
// and by the FH_ASSEMBLE_REPRODUCIBLE check (it used to hand-copy the conditions; scripts/kernel_selection_table.py tabulates the outcome).
enum GatherKernel { GK_ROWS_TET4, GK_HEX8_ROWS, GK_PIPELINED, GK_GENERIC };
static GatherKernel select_gather_kernel(fh_ctx* c, bool fast, bool* pipe_rules_out) {
    const bool pipe_rules = c->has_pipe && c->has_rules && c->elem_par && c->fast_ok && c->op == FH_LINEAR_ELASTIC;
    const bool lin = c->op == FH_LAPLACE || c->op == FH_LINEAR_ELASTIC;
    if (pipe_rules_out) *pipe_rules_out = pipe_rules;
    // Tet4 is affine: with uniform parameters any rule equals the one-point rule that carries the sum of its weights
    if (c->has_pipe && c->has_rows && c->elem_kind == FH_TET4 && (fast || pipe_rules) && lin) return GK_ROWS_TET4;
    if (c->has_pipe && c->has_hrows && fast && !pipe_rules && c->nq == 8 && c->elem_kind == FH_HEX8 && lin && !c->opt.NO_HEX8_ROWS &&
        hex8_rows_lds_bytes(c->g_acc) <= LDS_LIMIT)
        return GK_HEX8_ROWS;
    if (c->has_pipe && (fast || pipe_rules) && lin) return GK_PIPELINED;
    return GK_GENERIC;
}
// largest buffer of dense element matrices the two-pass form may allocate, in GB
static int two_pass_max_gb(const fh_ctx* c) { return c->opt.TWO_PASS_MAX_GB.value_or(96); }

int assemble_matrix_enqueue(fh_ctx* c, double* values_dev, int flags, bool reset) {
    const auto t_entry = std::chrono::steady_clock::now();
    const bool vt_entry = !c->has_partition && c->opt.VERBOSE;
    struct ExitPrint {   // FENRIS_HIP_VERBOSE: the first assembly of a context from entry to the end of its enqueueing
        bool on; std::chrono::steady_clock::time_point t0; hipStream_t st;
        ~ExitPrint() {
            if (!on) return;
            const double enq = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            (void)hipStreamSynchronize(st);
            std::fprintf(stderr, "[fenris_hip] set-up: first assembly enqueued after %7.1f ms, finished after %7.1f ms\n", enq,
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
    } exit_print{vt_entry, t_entry, c->stream};
    int rc = check_ready(c, "fh_assemble_matrix", true);
    if (rc) return rc;
    rc = expansion_blocks_matrix(c, "fh_assemble_matrix");
    if (rc) return rc;
    if (!values_dev) return c->fail(FH_BAD_ARGUMENT, "fh_assemble_matrix: values is null");
    const int mode = flags & FH_SCATTER_MASK;
    const int overwrite = (flags & FH_ASSEMBLE_OVERWRITE) ? 1 : 0;
    if (reset) rc = reset_status(c);
    if (rc) return rc;
    if (c->E == 0) return FH_OK;
    KArgs a;
    fill_common(c, a);
    a.vals = values_dev;
    a.overwrite = overwrite;
    const uint64_t nnz = (uint64_t)c->S() * c->S() * c->nnz_nodes;
    if (mode == FH_SCATTER_GATHER && c->row_hi < 0 && !c->opt.NO_TWO_PASS) {
        // two-pass owner-computes (dense element matrices, then a row gather) where recomputing the element prologue per
        // owning node block is the expensive part: high-order elements, and the nonlinear materials on any element
        // (measured, Hex8 128^3: NeoHookean 11.1 -> 9.2 ms, StVK 19.2 -> 10.0 ms; LinearElastic with per-point
        // parameters is faster one-pass: 5.7 vs 8.2 ms).  The dense buffer costs E (s n)^2 doubles: capped.
        const size_t dense_doubles = two_pass_dense_doubles(c);
        const double dense_gb = (double)dense_doubles * 8.0 / 1e9;
        const bool want = c->ei.n > 8 || op_depends_on_u(c->op) || c->opt.TWO_PASS;
        if (want && dense_gb <= (double)two_pass_max_gb(c)) {
            // the dense buffer is allocated here: when the device cannot hold it the one-pass gather below takes over
            if (c->ke_dense.n >= dense_doubles || c->ke_dense.alloc(dense_doubles) == hipSuccess)
                return assemble_two_pass(c, values_dev, overwrite);
            (void)hipGetLastError();
        }
    }
    if (mode == FH_SCATTER_GATHER) {
        const bool vt_first = !c->has_partition && c->opt.VERBOSE;
        const auto t_bp0 = std::chrono::steady_clock::now();
        if (vt_first) std::fprintf(stderr, "[fenris_hip] set-up: before build_partition               %7.1f ms\n",
                                   std::chrono::duration<double, std::milli>(t_bp0 - t_entry).count());
        rc = build_partition(c);
        if (rc) return rc;
        if (vt_first) {
            (void)hipStreamSynchronize(c->stream);
            std::fprintf(stderr, "[fenris_hip] set-up: build_partition in all              %7.1f ms\n",
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_bp0).count());
        }
        if (c->part_rows_only && !(c->has_pipe && c->has_rows && a.fast && (c->op == FH_LAPLACE || c->op == FH_LINEAR_ELASTIC) &&
                              !c->opt.TRACE)) {
            // these tables are for the row-owner kernel only (see build_partition); another kernel is about to run
            c->perm_failed = true;
            c->has_partition = false; ++c->struct_gen;
            rc = build_partition(c);
            if (rc) return rc;
        }
        if (c->nblk == 0) return FH_OK;  // empty row range
        if (flags & FH_ASSEMBLE_REPRODUCIBLE) {
            // the kernels that sum in a fixed order: k_affine_rows (all positions affine), k_gather_rows_tet4, k_hex8_rows; anything else
            // (k_gather_pipelined, the generic one-pass gather: LDS atomics in hardware order) goes two-pass
            const GatherKernel gk = select_gather_kernel(c, a.fast != 0, nullptr);
            const bool stable = c->npos_gen == 0 || gk == GK_ROWS_TET4 || gk == GK_HEX8_ROWS;
            if (!stable) {
                if (c->row_hi >= 0) return c->fail(FH_UNSUPPORTED, "FH_ASSEMBLE_REPRODUCIBLE: this configuration needs the two-pass form, which has no row range");
                const size_t dense_doubles = two_pass_dense_doubles(c);
                if ((double)dense_doubles * 8.0 / 1e9 > (double)two_pass_max_gb(c))
                    return c->fail(FH_OUT_OF_MEMORY, "FH_ASSEMBLE_REPRODUCIBLE: the dense element matrices of the two-pass form exceed FENRIS_HIP_TWO_PASS_MAX_GB");
                if (c->ke_dense.n < dense_doubles && c->ke_dense.alloc(dense_doubles) != hipSuccess) {
                    (void)hipGetLastError();
                    return c->fail(FH_OUT_OF_MEMORY, "FH_ASSEMBLE_REPRODUCIBLE: no device memory for the dense element matrices of the two-pass form");
                }
                return assemble_two_pass(c, values_dev, overwrite);
            }
        }
        c->last_kernel.clear();
        if (c->a_npos > 0) {
            // node blocks whose elements are all affine (affine_kernel.hpp); the remaining positions follow below
            rc = launch_affine(c, a);
            if (rc) return rc;
            c->last_kernel = "k_affine_rows";
            if (c->npos_gen == 0) return FH_OK;
            c->last_kernel += " + ";
        }
        a.blk_off = c->blk_off.p;
        a.gt_hdr = c->gt_hdr.p;
        a.gt_elems = c->gt_elems.p;
        a.gt_ent = c->gt_ent.p;
        a.gt_pos = c->has_pos ? c->gt_pos.p : nullptr;
        a.nblk = c->nblk;
        a.ub = c->g_ub;
        a.mb = c->g_mb;
        a.acc_max = c->g_acc;
        a.nb_max = c->g_nb;
        const size_t lds = layout_bytes_dyn(c->elem_kind, c->op, WHAT_MATRIX, c->nq, a.ub, a.acc_max, a.nb_max, true, a.mb, a.fast);
        bool pipe_rules = false;
        const GatherKernel gk = select_gather_kernel(c, a.fast != 0, &pipe_rules);
        if (pipe_rules && !c->has_slotpar) {
            const size_t n = (size_t)c->npos_gen * c->p_us;
            HIP_TRY(c, c->p_slotpar.alloc(2 * n));
            hipLaunchKernelGGL(k_build_slot_params, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->p_elem.p, n,
                               c->rule_map.p, c->rparams.p, c->nq, c->p_slotpar.p);
            HIP_TRY(c, hipGetLastError());
            c->has_slotpar = true;
        }
        // Tet4 is affine: gradients and det J are the same at every point, so with uniform parameters any rule equals the
        // one-point rule that carries the sum of its weights (the table of gradients at point 0 serves as is)
        if (gk == GK_ROWS_TET4) {
            a.fast = 1;
            if (c->nq > 1) {
                a.qw = c->qw.p + c->nq;
                a.nq = 1;
            }
            RowTablesS T{c->r_rec.p, c->r_lanes4.p, c->r_vconn.p, c->p_elem.p, pipe_rules ? c->p_slotpar.p : nullptr,
                         c->r_rw, c->p_us, c->p_nbs, c->npos_gen, c->r_ls, c->r_vn, c->opt.TET4_PRIO.value_or(0) & 15};
            a.ub = std::max(c->p_us, 76);   // the X region of the layout (14 doubles per slot) holds the vertex table: 256 x 4 doubles
            a.nb_max = c->p_nbs;
            if (c->has_mask && a.overwrite) {   // blocks without an active element have no lane: clear the range first (rows_kernel.hpp)
                const int n_lo = (c->row_hi < 0) ? 0 : (int)std::min<long long>(c->row_lo, (long long)c->N);
                const int n_hi = (c->row_hi < 0) ? (int)c->N : (int)std::min<long long>(c->row_hi, (long long)c->N);
                if (n_hi > n_lo) {
                    hipLaunchKernelGGL(k_zero_node_rows, dim3(2048), dim3(256), 0, c->stream, c->noff.p, n_lo, n_hi, c->S() * c->S(), values_dev);
                    HIP_TRY(c, hipGetLastError());
                }
            }
            c->last_kernel += "k_gather_rows";
            if (pipe_rules) return launch_rows_tet4<FH_LINEAR_ELASTIC, true>(c, a, T);
            return c->op == FH_LAPLACE ? launch_rows_tet4<FH_LAPLACE>(c, a, T) : launch_rows_tet4<FH_LINEAR_ELASTIC>(c, a, T);
        }
        if (gk == GK_HEX8_ROWS) {
            const size_t lds_h = hex8_rows_lds_bytes(c->g_acc);
            {
                const int per_cu = std::max(1, (int)std::min<size_t>(2, (LDS_LIMIT - 512) / std::max<size_t>(lds_h, 1)));
                const int grid = std::max(1, std::min(c->npos_gen, c->opt.PIPE_GRID.value_or(c->num_cus * c->opt.PIPE_WGS_PER_CU.value_or(per_cu))));
                // the deferred lane tuner: in front of the launch that follows the first FENRIS_HIP_TUNE_AFTER ones
                if (c->h_tune_pending > 0 && --c->h_tune_pending == 0) {
                    c->h_tune_pending = 1;
                    const int rt = hex8_tune_lanes_now(c);
                    if (rt) return rt;
                }
                Hex8RowTables T{c->h_pos.p, c->h_lanes.p, c->p_conn.p, c->p_elem.p, c->p_us, c->p_cs, c->npos_gen, c->g_acc};
                if (c->opt.VERBOSE)
                    std::fprintf(stderr, "[fenris_hip] hex8 rows: positions %d lds=%zu B wgs/cu=%d grid=%d\n", c->npos_gen, lds_h, per_cu, grid);
                c->last_kernel += "k_hex8_rows";
                HIP_TRY(c, hex8_rows_launch(c->op, grid, lds_h, c->stream, a, T, a.ablate | (a.trace ? 0x10000 : 0) | ((c->opt.HEX8_PRIO.value_or(40) & 63) << HEX8_ROWS_PRIO_SHIFT)));
                return FH_OK;
            }
        }
        if (gk == GK_PIPELINED) {
            a.fast = 1;
            PipeTables T{c->p_rec.p, c->p_conn.p, c->p_elem.p, pipe_rules ? c->p_slotpar.p : nullptr, c->p_rw,
                         c->p_cs, c->p_ms, c->p_nbs, c->p_us, c->npos_gen};
            a.ub = c->p_us;  // LDS slots: every unique element of a block is staged, shared ones persist
            a.mb = c->p_ms;  // the LDS layout is sized by the table strides
            a.nb_max = c->p_nbs;
            c->last_kernel += "k_gather_pipelined";
            return launch_pipelined(c, a, T, 0, 0);
        }
        c->last_kernel += "k_assemble_matrix<gather>";
        return launch_matrix_dyn(c, a, MODE_GATHER, lds, c->nblk);
    }
    if (c->row_hi >= 0) return c->fail(FH_UNSUPPORTED, "fh_assemble_matrix: a row range needs FH_SCATTER_GATHER");
    if (overwrite) HIP_TRY(c, hipMemsetAsync(values_dev, 0, sizeof(double) * nnz, c->stream));
    a.epb = choose_epb(c, WHAT_MATRIX);
    a.ub = a.epb;
    // high-order elements: column search of the scatter in LDS (neighbour lists staged per element)
    if (c->ei.n > 8) {
        const unsigned max_row = c->max_row;
        const size_t with_nc = layout_bytes_dyn(c->elem_kind, c->op, WHAT_MATRIX, c->nq, a.ub, 0, 0, false, 0, a.fast, (int)max_row);
        if (with_nc <= LDS_TARGET + 16 * 1024) a.nc_row = (int)max_row;
    }
    const size_t lds = layout_bytes_dyn(c->elem_kind, c->op, WHAT_MATRIX, c->nq, a.ub, 0, 0, false, 0, a.fast, a.nc_row);
    if (lds > LDS_LIMIT) return c->fail(FH_UNSUPPORTED, "quadrature rule too large for LDS staging");
    if (mode == FH_SCATTER_ATOMIC) {
        if (flags & FH_ASSEMBLE_REPRODUCIBLE) return c->fail(FH_BAD_ARGUMENT, "FH_ASSEMBLE_REPRODUCIBLE: fp64 atomics add in hardware order; use FH_SCATTER_GATHER or FH_SCATTER_COLORED");
        a.work_begin = 0;
        a.work_end = (long long)(c->has_mask ? c->num_active : c->E);
        a.labels = c->has_mask ? c->active_list.p : nullptr;
        if (a.work_end == 0) return FH_OK;
        const int grid = (int)((a.work_end + a.epb - 1) / a.epb);
        c->last_kernel = "k_assemble_matrix<atomic>";
        return launch_matrix_dyn(c, a, MODE_ATOMIC, lds, grid);
    }
    if (mode == FH_SCATTER_COLORED) {
        if (!c->has_colors) return c->fail(FH_INVALID_STATE, "FH_SCATTER_COLORED: call fh_color or fh_set_colors first");
        a.labels = c->labels.p;
        c->last_kernel = "k_assemble_matrix<colored>";
        for (size_t col = 0; col + 1 < c->color_offsets.size(); ++col) {
            a.work_begin = (long long)c->color_offsets[col];
            a.work_end = (long long)c->color_offsets[col + 1];
            const long long cntc = a.work_end - a.work_begin;
            if (cntc <= 0) continue;
            const int grid = (int)((cntc + a.epb - 1) / a.epb);
            rc = launch_matrix_dyn(c, a, MODE_COLORED, lds, grid);
            if (rc) return rc;
        }
        return FH_OK;
    }
    return c->fail(FH_BAD_ARGUMENT, "fh_assemble_matrix: unknown scatter mode");
}

extern "C" {
static bool mode_is_colored(int flags) { return (flags & FH_SCATTER_MASK) == FH_SCATTER_COLORED; }
int fh_assemble_matrix_async_dev(fh_ctx* c, double* values_dev, int flags) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->rs.active) return assemble_matrix_enqueue(c, values_dev, flags);
    // rule-set table: one pass per group of rules, the first one with the caller's flags, the others accumulating
    int rc = check_ready(c, "fh_assemble_matrix", true);
    if (rc) return rc;
    rc = expansion_blocks_matrix(c, "fh_assemble_matrix");
    if (rc) return rc;
    if (!values_dev) return c->fail(FH_BAD_ARGUMENT, "fh_assemble_matrix: values is null");
    rc = reset_status(c);
    if (rc) return rc;
    bool any = false;
    rc = rs_for_each_group(c, [&](bool first) {
        any = true;
        if (mode_is_colored(flags) && !c->has_colors) return c->fail(FH_INVALID_STATE, "fh_assemble_matrix: FH_SCATTER_COLORED needs fh_color / fh_set_colors");
        return assemble_matrix_enqueue(c, values_dev, first ? flags : (flags & ~FH_ASSEMBLE_OVERWRITE), false);
    });
    if (rc) return rc;
    if (!any && (flags & FH_ASSEMBLE_OVERWRITE) && fh_nnz(c))
        HIP_TRY(c, hipMemsetAsync(values_dev, 0, sizeof(double) * fh_nnz(c), c->stream));
    return FH_OK;
}

// ---- placement of the streamed buffers (round 3).  The time of the owner-computes kernels follows how the large buffers they stream
// through happen to be backed by device memory -- the same context, kernel and arguments run in one of two or three levels up to 10 %
// apart depending only on WHICH physical memory a buffer got (re-allocating a buffer at the same virtual address changes the level;
// profiles/r03_affine_experiments.txt, section 7).  Nothing in the HIP API chooses the backing, so the library offers the only remedy
// there is: time the real assembly and keep the better of several allocations.
int fh_time_assembly_dev(fh_ctx* c, double* values_dev, int flags, int reps, double* ms_per_assembly) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (!ms_per_assembly || reps < 1) return c->fail(FH_BAD_ARGUMENT, "fh_time_assembly_dev: bad argument");
    // reps + 1 REAL assemblies run into the caller's array: without FH_ASSEMBLE_OVERWRITE they would pile up reps + 1 copies of K
    if (!(flags & FH_ASSEMBLE_OVERWRITE)) return c->fail(FH_BAD_ARGUMENT, "fh_time_assembly_dev: needs FH_ASSEMBLE_OVERWRITE (the timed assemblies write the values)");
    c->a_shared_now = true;   // the tables of the shared affine loader belong to this set-up assembly, not into the timed ones
    int rc = fh_assemble_matrix_async_dev(c, values_dev, flags);   // tables, code objects, first touch
    c->a_shared_now = false;
    if (rc) return rc;
    // the deferred lane tuner of k_hex8_rows (host work in front of a later launch) belongs to the set-up, not into the timed assemblies --
    // nor into the baseline fh_tune_placement_dev compares its candidates with
    if (c->h_tune_pending > 0) { rc = hex8_tune_lanes_now(c); if (rc) return rc; }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t he = hipEventCreate(&e0);
    if (he == hipSuccess) he = hipEventCreate(&e1);
    if (he == hipSuccess) he = hipEventRecord(e0, c->stream);
    if (he != hipSuccess) {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        return c->hip_fail(he, "fh_time_assembly_dev");
    }
    for (int k = 0; k < reps && rc == FH_OK; ++k) rc = fh_assemble_matrix_async_dev(c, values_dev, flags);
    he = hipEventRecord(e1, c->stream);
    if (he == hipSuccess) he = hipEventSynchronize(e1);
    float ms = 0.f;
    if (he == hipSuccess) he = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (rc) return rc;
    if (he != hipSuccess) return c->hip_fail(he, "fh_time_assembly_dev");
    *ms_per_assembly = (double)ms / reps;
    uint64_t failed = 0;
    return fh_poll_status(c, &failed);
}

int fh_tune_placement_dev(fh_ctx* c, double* values_dev, int flags, int tries, double* ms_before, double* ms_after) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (!(flags & FH_ASSEMBLE_OVERWRITE)) return c->fail(FH_BAD_ARGUMENT, "fh_tune_placement_dev: needs FH_ASSEMBLE_OVERWRITE (the trial assemblies write the values)");
    double best = 0.0;
    int rc = fh_time_assembly_dev(c, values_dev, flags, 3, &best);
    if (rc) return rc;
    if (ms_before) *ms_before = best;
    if (ms_after) *ms_after = best;
    // the one large buffer of its own that the affine kernels stream through: the element records.  (Moving the position tables and
    // the lane tables never changed the level.)  Rejected allocations are held until the end: freed at once they would be handed out again.
    // A candidate holds no records: every exchange of the pointer, the return to the old buffer included, moves a_recs_gen, so the first of
    // the reps + 1 assemblies of each timing forms them and the timed ones read them.  The candidates are ranked by the sweep's reads of the
    // buffer, which is what its placement changes.
    if (!c->a_recs.p || c->a_npos == 0 || tries < 1) return FH_OK;
    std::vector<double*> rejected;
    const size_t bytes = c->a_recs.n * sizeof(double);
    for (int k = 0; k < tries; ++k) {
        double* cand = nullptr;
        if (hipMalloc(reinterpret_cast<void**>(&cand), bytes) != hipSuccess) { (void)hipGetLastError(); break; }
        double* old = c->a_recs.p;
        c->a_recs.p = cand;
        ++c->a_recs_gen;
        double t = 0.0;
        rc = fh_time_assembly_dev(c, values_dev, flags, 3, &t);
        // (FENRIS_HIP_PLACEMENT_KEEP=1, TESTS ONLY -- declared as such in options.def: every candidate is kept whatever its time, so
        // that a test can hold an assembly behind an exchange against the one before it; it makes the placement worse)
        if (rc == FH_OK && (t < 0.98 * best || c->opt.PLACEMENT_KEEP.value_or(0))) {
            best = t;
            rejected.push_back(old);
        } else {
            c->a_recs.p = old;   // (its records were current before the exchange, but nothing remembers that: formed again by the next assembly)
            ++c->a_recs_gen;
            rejected.push_back(cand);
        }
        if (rc) break;
    }
    (void)hipStreamSynchronize(c->stream);
    for (double* p : rejected) (void)hipFree(p);
    if (ms_after) *ms_after = best;
    return rc;
}

// The rows of the nodes [node_begin, node_end) with a second set of owner-computes tables; the context's own row range and
// tables are untouched.  The second set is built on first use and rebuilt when the range or anything the tables depend on
// (mesh, pattern, mask, operator, quadrature, affine classes) has changed since.
int fh_assemble_matrix_rows_async_dev(fh_ctx* c, double* values_dev, int flags, uint64_t node_begin, uint64_t node_end) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->has_mesh || c->ragged) return c->fail(FH_INVALID_STATE, "fh_assemble_matrix_rows: set the mesh first");
    if (node_begin > node_end || node_end > c->N) return c->fail(FH_BAD_ARGUMENT, "fh_assemble_matrix_rows: bad node range");
    if ((flags & FH_SCATTER_MASK) != FH_SCATTER_GATHER) return c->fail(FH_UNSUPPORTED, "fh_assemble_matrix_rows: needs FH_SCATTER_GATHER");
    if (c->rs.active) return c->fail(FH_UNSUPPORTED, "fh_assemble_matrix_rows: not with a rule-set quadrature table");
    if (!c->rows_stash) c->rows_stash = new PartStash();
    PartStash& st = *c->rows_stash;
    swap_partition(c, st);   // the context's own tables wait in the stash
    if (st.built_gen != c->struct_gen || c->row_lo != (long long)node_begin || c->row_hi != (long long)node_end) {
        c->row_lo = (long long)node_begin;   // a range, even when it covers every node: the two-pass path does not apply
        c->row_hi = (long long)node_end;
        c->has_partition = false;
        c->aff_failed = false;
    }
    c->status_slot = 1;
    const int rc = assemble_matrix_enqueue(c, values_dev, flags);
    c->status_slot = 0;
    swap_partition(c, st);
    st.built_gen = rc ? ~0ull : c->struct_gen;
    return rc;
}

int fh_assemble_matrix_rows_dev(fh_ctx* c, double* values_dev, int flags, uint64_t node_begin, uint64_t node_end, uint64_t* failed) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    const int rc = fh_assemble_matrix_rows_async_dev(c, values_dev, flags, node_begin, node_end);
    if (rc) return rc;
    return read_status(c, failed);
}

int fh_poll_status(fh_ctx* c, uint64_t* failed) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    return read_status(c, failed);
}

int fh_assemble_matrix_dev(fh_ctx* c, double* values_dev, int flags, uint64_t* failed) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int rc = fh_assemble_matrix_async_dev(c, values_dev, flags);
    if (rc) return rc;
    return read_status(c, failed);
}

int fh_assemble_matrix(fh_ctx* c, double* values, int flags, uint64_t* failed) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int rc = check_ready(c, "fh_assemble_matrix", true);
    if (rc) return rc;
    rc = expansion_blocks_matrix(c, "fh_assemble_matrix");
    if (rc) return rc;
    if (!values) return c->fail(FH_BAD_ARGUMENT, "fh_assemble_matrix: values is null");
    const uint64_t nnz = fh_nnz(c);
    DevBuf<double> d;
    HIP_TRY(c, d.alloc((size_t)nnz));
    // the staging copy starts from the caller's values unless every entry is about to be overwritten: with a row range
    // (fh_set_row_range) FH_ASSEMBLE_OVERWRITE writes the rows in range only, "the others are left untouched"
    if (!(flags & FH_ASSEMBLE_OVERWRITE) || c->row_hi >= 0)
        HIP_TRY(c, hipMemcpyAsync(d.p, values, sizeof(double) * nnz, hipMemcpyHostToDevice, c->stream));
    rc = fh_assemble_matrix_dev(c, d.p, flags, failed);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(values, d.p, sizeof(double) * nnz, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FH_OK;
}

int fh_assemble_element_matrices_dev(fh_ctx* c, uint64_t first, uint64_t count, double* ke_dev) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int rc = check_ready(c, "fh_assemble_element_matrices", false);
    if (rc) return rc;
    rc = expansion_blocks_matrix(c, "fh_assemble_element_matrices");
    if (rc) return rc;
    if (first + count > c->E || (count && !ke_dev)) return c->fail(FH_BAD_ARGUMENT, "fh_assemble_element_matrices: bad range");
    if (count == 0) return FH_OK;
    rc = reset_status(c);
    if (rc) return rc;
    if (c->rs.active) {  // rule-set table: runs of consecutive elements whose rules share points and weights
        const size_t ld = (size_t)c->S() * c->ei.n;
        for (uint64_t e0 = first; e0 < first + count && rc == FH_OK;) {
            const int g = c->rs.rule_group[c->rs.e2r[e0]];
            uint64_t e1 = e0 + 1;
            while (e1 < first + count && c->rs.rule_group[c->rs.e2r[e1]] == g) ++e1;
            if (c->rs.staged != g) rc = rs_stage(c, g);
            if (rc == FH_OK) rc = element_matrices_enqueue(c, e0, e1 - e0, ke_dev + ld * ld * (e0 - first), false);
            e0 = e1;
        }
        const int rc2 = apply_mask(c, c->user_has_mask ? c->user_mask.data() : nullptr);
        if (rc || rc2) return rc ? rc : rc2;
        return read_status(c, nullptr);
    }
    rc = element_matrices_enqueue(c, first, count, ke_dev, false);
    if (rc) return rc;
    return read_status(c, nullptr);
}

int fh_assemble_element_matrices(fh_ctx* c, uint64_t first, uint64_t count, double* ke_out) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int rc = check_ready(c, "fh_assemble_element_matrices", false);
    if (rc) return rc;
    rc = expansion_blocks_matrix(c, "fh_assemble_element_matrices");
    if (rc) return rc;
    if (first + count > c->E || (count && !ke_out)) return c->fail(FH_BAD_ARGUMENT, "fh_assemble_element_matrices: bad range");
    if (count == 0) return FH_OK;
    const size_t ld = (size_t)c->S() * c->ei.n;
    DevBuf<double> d;
    HIP_TRY(c, d.alloc(ld * ld * count));
    rc = fh_assemble_element_matrices_dev(c, first, count, d.p);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(ke_out, d.p, sizeof(double) * ld * ld * count, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FH_OK;
}

// the groups of a rule-set table one after the other; every pass accumulates.  The lowest failing element over all groups
// is reported, like the serial loop of the reference would (global.rs:154: first error aborts).
}  // extern "C"
