// Recovery of gradient, strain, stress, energy density and measure at points, elements and nodes: launchers and C ABI (recover_kernels.hpp)
#include "engine_internal.hpp"
#include "recover_kernels.hpp"

static bool low_order(int kind) { return kind == FH_QUAD4 || kind == FH_HEX8 || kind == FH_TET4 || kind == FH_TRI3; }

// components of `quantity` for the context's operator; the checks shared by every entry point (arguments first, then the state)
static int recover_check(fh_ctx* c, const char* who, int quantity, uint32_t* ncomp) {
    if (quantity < FH_RECOVER_GRAD_U || quantity > FH_RECOVER_VOLUME) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": unknown quantity");
    if (!c->has_mesh || c->ragged) return c->fail(FH_INVALID_STATE, std::string(who) + ": no finite element mesh set");
    if (c->op < 0) return c->fail(FH_INVALID_STATE, std::string(who) + ": no operator set");
    if (!op_has_stress(c->op)) return c->fail(FH_UNSUPPORTED, std::string(who) + ": the mass operators and FH_TENSOR have no recovered quantities");
    const int d = c->ei.d, s = c->S();
    const bool solid = quantity == FH_RECOVER_STRAIN || quantity == FH_RECOVER_STRESS_CAUCHY || quantity == FH_RECOVER_VON_MISES;
    if (c->op == FH_LAPLACE && solid) return c->fail(FH_UNSUPPORTED, std::string(who) + ": FH_LAPLACE has no strain, Cauchy or von Mises stress");
    if (ncomp)
        *ncomp = quantity == FH_RECOVER_GRAD_U ? d * s : (quantity == FH_RECOVER_STRAIN || quantity == FH_RECOVER_STRESS_CAUCHY) ? d * d
               : quantity == FH_RECOVER_STRESS_PK1 ? s * d : 1;
    return FH_OK;
}
static int recover_where_check(fh_ctx* c, const char* who, int where) {
    if (where < FH_AT_POINTS || where > FH_AT_NODES) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": unknown location");
    return FH_OK;
}
static int recover_table_check(fh_ctx* c, const char* who) {
    if (c->rs.active) return c->fail(FH_UNSUPPORTED, std::string(who) + ": rule-set quadrature tables (fh_set_quadrature_rules) are not walked here");
    if (c->nq <= 0) return c->fail(FH_INVALID_STATE, std::string(who) + ": no quadrature table set");
    return FH_OK;
}

// one pass over the elements: thread per element (mean / volume of the small iso-parametric kinds) or thread per (element, point)
static int launch_recover_elements(fh_ctx* c, const KArgs& a, const RecoverArgs& r, int quantity, bool per_element) {
    const int op = quantity == FH_RECOVER_VOLUME ? (int)FH_LAPLACE : c->op;   // the measure needs no operator: one instantiation per kind
    const long long threads = per_element ? a.num_elements : a.num_elements * a.nq;
    const long long grid = (threads + 255) / 256;
    if (grid > 0x7fffffffll) return c->fail(FH_UNSUPPORTED, "fh_recover: more than 2^31 workgroups");
    return dispatch(all_kinds, c->elem_kind, elliptic_ops, op, (int)FH_UNSUPPORTED, [&](auto ek, auto opc) {
        return dispatch(recover_quantities, quantity, (int)FH_BAD_ARGUMENT, [&](auto q) {
            if constexpr (!recover_defined<opc(), q()>) {
                return (int)FH_UNSUPPORTED;
            } else {
                // (the expansion: its own instantiations of the quantities that come from the elastic part, the others as they were)
                return dispatch_bool(recover_expands<opc(), q()> && a.theta != nullptr, [&](auto ex) {
                    constexpr bool EX = ex() && recover_expands<opc(), q()>;
                    if constexpr (ElemT<ek()>::N == ElemT<ek()>::NG) {
                        if (per_element) {
                            hipLaunchKernelGGL((k_recover_elements<ek(), opc(), q(), FH_AT_ELEMENTS, EX>), dim3((unsigned)grid), dim3(256), 0, c->stream, a, r);
                            HIP_TRY(c, hipGetLastError());
                            return (int)FH_OK;
                        }
                    }
                    hipLaunchKernelGGL((k_recover_elements<ek(), opc(), q(), FH_AT_POINTS, EX>), dim3((unsigned)grid), dim3(256), 0, c->stream, a, r);
                    HIP_TRY(c, hipGetLastError());
                    return (int)FH_OK;
                });
            }
        });
    });
}

extern "C" {

int fh_recover_components(fh_ctx* c, int quantity, uint32_t* ncomp) {
    if (!c) return FH_BAD_ARGUMENT;
    if (!ncomp) return c->fail(FH_BAD_ARGUMENT, "fh_recover_components: ncomp is null");
    return recover_check(c, "fh_recover_components", quantity, ncomp);
}

int fh_recover_rows(fh_ctx* c, int where, uint64_t* rows) {
    if (!c) return FH_BAD_ARGUMENT;
    if (!rows) return c->fail(FH_BAD_ARGUMENT, "fh_recover_rows: rows is null");
    int rc = recover_where_check(c, "fh_recover_rows", where);
    if (rc) return rc;
    if (!c->has_mesh || c->ragged) return c->fail(FH_INVALID_STATE, "fh_recover_rows: no finite element mesh set");
    if (where == FH_AT_POINTS) {
        rc = recover_table_check(c, "fh_recover_rows");
        if (rc) return rc;
    }
    *rows = where == FH_AT_POINTS ? c->E * (uint64_t)c->nq : where == FH_AT_ELEMENTS ? c->E : c->N;
    return FH_OK;
}

int fh_recover_dev(fh_ctx* c, int quantity, int where, double* out_dev) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    uint32_t ncomp = 0;
    if (quantity < FH_RECOVER_GRAD_U || quantity > FH_RECOVER_VOLUME) return c->fail(FH_BAD_ARGUMENT, "fh_recover: unknown quantity");
    int rc = recover_where_check(c, "fh_recover", where);
    if (rc) return rc;
    if (quantity == FH_RECOVER_VOLUME && where != FH_AT_ELEMENTS) return c->fail(FH_BAD_ARGUMENT, "fh_recover: FH_RECOVER_VOLUME is defined at FH_AT_ELEMENTS only");
    rc = recover_check(c, "fh_recover", quantity, &ncomp);
    if (rc) return rc;
    rc = expansion_blocked(c, "fh_recover");
    if (rc) return rc;
    rc = recover_table_check(c, "fh_recover");
    if (rc) return rc;
    if (c->op != FH_LAPLACE && !c->has_params) return c->fail(FH_INVALID_STATE, "fh_recover: operator needs per-point parameters (mu, lambda)");
    const size_t E = (size_t)c->E, nq = (size_t)c->nq, nc = ncomp;
    const size_t rows = where == FH_AT_POINTS ? E * nq : where == FH_AT_ELEMENTS ? E : (size_t)c->N;
    if (!out_dev && rows > 0) return c->fail(FH_BAD_ARGUMENT, "fh_recover: out is null");
    if (where == FH_AT_NODES && c->N > 0 && E == 0) {
        HIP_TRY(c, hipMemsetAsync(out_dev, 0, sizeof(double) * (size_t)c->N * nc, c->stream));
        return FH_OK;
    }
    if (E == 0) return FH_OK;
    rc = reset_status(c);
    if (rc) return rc;
    KArgs a;
    fill_common(c, a);
    RecoverArgs r{};
    r.active = c->has_mask ? c->active.p : nullptr;
    const bool low = low_order(c->elem_kind), nodes = where == FH_AT_NODES, volume = quantity == FH_RECOVER_VOLUME;
    // scratch: [element means | element volumes] of a nodal request, [point rows | point measures] of the quadratic kinds' means
    const bool two_step = where != FH_AT_POINTS && !low;
    const size_t n_mean = nodes ? E * nc : 0, n_vol = nodes ? E : 0, n_pts = (two_step && !volume) ? E * nq * nc : 0, n_meas = two_step ? E * nq : 0;
    const size_t need = n_mean + n_vol + n_pts + n_meas;
    if (need > 0 && c->recover_scratch.n < need) HIP_TRY(c, c->recover_scratch.alloc(need));
    double* s_mean = c->recover_scratch.p;
    double* s_vol = s_mean + n_mean;
    double* s_pts = s_vol + n_vol;
    double* s_meas = s_pts + n_pts;
    if (where == FH_AT_POINTS) {
        r.points = out_dev;
        rc = launch_recover_elements(c, a, r, quantity, false);
        if (rc) return rc;
        c->last_kernel = "k_recover_elements<points>";
    } else {
        double* mean = nodes ? s_mean : (volume ? nullptr : out_dev);
        double* vol = nodes ? s_vol : (volume ? out_dev : nullptr);
        if (low) {
            r.mean = mean;
            r.volume = vol;
            rc = launch_recover_elements(c, a, r, quantity, true);
            if (rc) return rc;
            c->last_kernel = "k_recover_elements<elements>";
        } else {
            r.points = volume ? nullptr : s_pts;
            r.measure = s_meas;
            rc = launch_recover_elements(c, a, r, quantity, false);
            if (rc) return rc;
            const long long grid = ((long long)(E * nc) + 255) / 256;
            if (grid > 0x7fffffffll) return c->fail(FH_UNSUPPORTED, "fh_recover: more than 2^31 workgroups");
            hipLaunchKernelGGL(k_recover_means, dim3((unsigned)grid), dim3(256), 0, c->stream, (long long)E, (int)nq, (int)nc, r.active, r.points, s_meas,
                               mean, vol);
            HIP_TRY(c, hipGetLastError());
            c->last_kernel = "k_recover_elements<points> + k_recover_means";
        }
        if (nodes) {
            // the node -> (element, local node) adjacency: the pattern's when there is one, else the source assembler's
            const unsigned *adj_off = c->n2e_off.p, *adj = c->n2e.p;
            if (!c->has_pattern) {
                rc = build_source_adjacency(c);
                if (rc) return rc;
                adj_off = c->src_n2e_off.p;
                adj = c->src_n2e.p;
            }
            const int grid = (int)(((long long)c->N + 255) / 256);
            rc = dispatch(recover_components, (int)nc, (int)FH_UNSUPPORTED, [&](auto ncc) {
                hipLaunchKernelGGL(k_recover_nodes<ncc()>, dim3(grid), dim3(256), 0, c->stream, (int)c->N, c->ei.n, adj_off, adj, r.active, s_mean, s_vol,
                                   out_dev);
                HIP_TRY(c, hipGetLastError());
                return (int)FH_OK;
            });
            if (rc) return rc;
            c->last_kernel += " + k_recover_nodes";
        }
    }
    return read_status(c, nullptr);
}

int fh_recover(fh_ctx* c, int quantity, int where, double* out) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    uint32_t ncomp = 0;
    uint64_t rows = 0;
    if (quantity < FH_RECOVER_GRAD_U || quantity > FH_RECOVER_VOLUME) return c->fail(FH_BAD_ARGUMENT, "fh_recover: unknown quantity");
    int rc = recover_where_check(c, "fh_recover", where);
    if (rc) return rc;
    if (quantity == FH_RECOVER_VOLUME && where != FH_AT_ELEMENTS) return c->fail(FH_BAD_ARGUMENT, "fh_recover: FH_RECOVER_VOLUME is defined at FH_AT_ELEMENTS only");
    rc = recover_check(c, "fh_recover", quantity, &ncomp);
    if (rc) return rc;
    rc = recover_table_check(c, "fh_recover");
    if (rc) return rc;
    rc = fh_recover_rows(c, where, &rows);
    if (rc) return rc;
    if (!out && rows > 0) return c->fail(FH_BAD_ARGUMENT, "fh_recover: out is null");
    const size_t len = (size_t)rows * ncomp;
    DevBuf<double> d;
    HIP_TRY(c, d.alloc(len + 1));
    rc = fh_recover_dev(c, quantity, where, d.p);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(out, d.p, sizeof(double) * len, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FH_OK;
}

}  // extern "C"
