// Per-element expansion (fh_set_element_expansion, fh_set_thermal_expansion, fh_element_expansion): one isotropic stress-free stretch
// theta_e > 0 per element, which strains the four elastic operators on every element-to-node route (material.hpp, Stretch, has the law).
// The field lives in the context (fh_ctx::expansion), reaches the kernels through KArgs::theta (fill_common) and is dropped by fh_set_mesh*;
// setting or clearing it moves expansion_gen, which the caches that depend on u or on the material carry in their keys (expansion_key).
// The routes that cannot honour it refuse while it is set (expansion_blocked, expansion_blocks_matrix).
#include "engine_internal.hpp"

namespace {

// theta_e = 1 + alpha_e (mean of the element's nodal temperatures, summed in local node order, - T_ref); a value that is not finite or not
// positive leaves the lowest such element in *bad
__global__ void __launch_bounds__(256) k_thermal_stretch(const int* conn, int n, long long E, const double* T, const double* alpha, int alpha_per_elem,
                                                         double T_ref, double* theta, unsigned long long* bad /* [0]: lowest offending element, [1]: any stretch != 1 */) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    double sum = 0.0;
    for (int a = 0; a < n; ++a) sum += T[conn[(size_t)e * n + a]];
    const double th = 1.0 + alpha[alpha_per_elem ? e : 0] * (sum / (double)n - T_ref);
    theta[e] = th;
    if (th != 1.0) bad[1] = 1ull;   // (a field that is not the identity)
    if (!(th > 0.0) || !(th <= 1.7976931348623157e308)) atomicMin(bad, (unsigned long long)e);
}

__global__ void __launch_bounds__(256) k_negate(long long n, double* v) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) v[i] = -v[i];
}

std::string bad_stretch(const char* who, uint64_t e, double v) {
    char buf[160];
    std::snprintf(buf, sizeof buf, "%s: the expansion of element %llu is %g; a stretch must be finite and positive", who, (unsigned long long)e, v);
    return buf;
}

int set_ready(fh_ctx* c, const char* who) {
    if (c->ragged) return c->fail(FH_UNSUPPORTED, std::string(who) + ": the element expansion does not cover ragged connectivity");
    if (!c->has_mesh) return c->fail(FH_INVALID_STATE, std::string(who) + ": no finite element mesh set");
    return FH_OK;
}

void clear(fh_ctx* c) {
    if (c->expansion_n) ++c->expansion_gen;
    c->expansion_n = 0;
}

// the checked stretches (host copy h, `count` of them) become the field: copied into a buffer of their own first, so that a failed allocation
// or copy leaves the standing field as it was
int install(fh_ctx* c, const double* src, hipMemcpyKind kind, const std::vector<double>* h, const double* host, uint64_t count) {
    bool identity = true;
    for (uint64_t e = 0; e < count; ++e) identity = identity && (h ? (*h)[e] : host[e]) == 1.0;
    DevBuf<double> th;
    HIP_TRY(c, th.alloc((size_t)count));
    HIP_TRY(c, hipMemcpyAsync(th.p, src, sizeof(double) * count, kind, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::swap(c->expansion.p, th.p);
    std::swap(c->expansion.n, th.n);
    c->expansion_identity = identity;
    c->expansion_n = count;
    ++c->expansion_gen;
    return FH_OK;
}

}  // namespace

// FH_UNSUPPORTED while a field is set and the route of `who` cannot honour it: FH_LAPLACE and FH_TENSOR have no elastic strain, rule-set
// tables are walked group by group with the element ids of a group.  The mass operators ignore the field.
int expansion_blocked(fh_ctx* c, const char* who) {
    if (!c->expansion_n) return FH_OK;
    if (c->op == FH_LAPLACE || c->op == FH_TENSOR)
        return c->fail(FH_UNSUPPORTED, std::string(who) + ": the element expansion (fh_set_element_expansion) strains the elastic operators only, not FH_LAPLACE "
                                                          "or FH_TENSOR; clear it first");
    if (c->rs.active)
        return c->fail(FH_UNSUPPORTED, std::string(who) + ": the element expansion (fh_set_element_expansion) does not cover rule-set quadrature tables "
                                                          "(fh_set_quadrature_rules)");
    return FH_OK;
}
// ... and the assembled stiffness of a hyperelastic operator; every other matrix is unaffected (the tangent of FH_LINEAR_ELASTIC does not see
// the field, the other operators have no elastic strain)
int expansion_blocks_matrix(fh_ctx* c, const char* who) {
    if (!c->expansion_n || !op_depends_on_u(c->op)) return FH_OK;
    return c->fail(FH_UNSUPPORTED, std::string(who) + ": the assembled stiffness of a hyperelastic operator does not carry the element expansion "
                                                      "(fh_set_element_expansion); use the matrix-free tangent");
}
// ... and FH_PRECOND_MULTIGRID: the coarse contexts of a hyperelastic operator would need the field restricted to them
int expansion_blocks_multigrid(fh_ctx* c, const char* who) {
    if (!c->expansion_n || !op_depends_on_u(c->op)) return FH_OK;
    return c->fail(FH_UNSUPPORTED, std::string(who) + ": FH_PRECOND_MULTIGRID with a hyperelastic operator does not carry the element expansion "
                                                      "(fh_set_element_expansion) to its coarse levels");
}
void expansion_drop(fh_ctx* c) { clear(c); }

extern "C" {

int fh_set_element_expansion_dev(fh_ctx* c, const double* theta_dev, uint64_t count) {
    const char* who = "fh_set_element_expansion";
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (!theta_dev || count == 0) { clear(c); return FH_OK; }
    int rc = set_ready(c, who);
    if (rc) return rc;
    if (count != 1 && count != c->E) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": count must be 1, the number of elements, or 0 to clear the expansion");
    std::vector<double> h((size_t)count);   // (the check is the host's: the values are few bytes per element and set once per load step)
    HIP_TRY(c, hipMemcpyAsync(h.data(), theta_dev, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (uint64_t e = 0; e < count; ++e)
        if (!(h[e] > 0.0) || !std::isfinite(h[e])) return c->fail(FH_BAD_ARGUMENT, bad_stretch(who, e, h[e]));
    return install(c, theta_dev, hipMemcpyDeviceToDevice, &h, nullptr, count);
}

int fh_set_element_expansion(fh_ctx* c, const double* theta, uint64_t count) {
    const char* who = "fh_set_element_expansion";
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (!theta || count == 0) { clear(c); return FH_OK; }
    int rc = set_ready(c, who);
    if (rc) return rc;
    if (count != 1 && count != c->E) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": count must be 1, the number of elements, or 0 to clear the expansion");
    for (uint64_t e = 0; e < count; ++e)
        if (!(theta[e] > 0.0) || !std::isfinite(theta[e])) return c->fail(FH_BAD_ARGUMENT, bad_stretch(who, e, theta[e]));
    return install(c, theta, hipMemcpyHostToDevice, nullptr, theta, count);
}

int fh_set_thermal_expansion_dev(fh_ctx* c, const double* T_nodes_dev, const double* alpha_dev, uint64_t alpha_count, double T_ref) {
    const char* who = "fh_set_thermal_expansion";
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int rc = set_ready(c, who);
    if (rc) return rc;
    if (!T_nodes_dev || !alpha_dev) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null argument");
    if (alpha_count != 1 && alpha_count != c->E) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": alpha_count must be 1 or the number of elements");
    if (!std::isfinite(T_ref)) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": T_ref must be finite");
    if (c->E == 0) { clear(c); return FH_OK; }
    // into a buffer of its own: a refused field leaves the standing one as it was
    DevBuf<double> th;
    DevBuf<unsigned long long> bad;
    HIP_TRY(c, th.alloc((size_t)c->E));
    HIP_TRY(c, bad.alloc(2));
    HIP_TRY(c, hipMemsetAsync(bad.p, 0xff, sizeof(unsigned long long), c->stream));
    HIP_TRY(c, hipMemsetAsync(bad.p + 1, 0, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(k_thermal_stretch, dim3((unsigned)((c->E + 255) / 256)), dim3(256), 0, c->stream, c->conn.p, c->ei.n, (long long)c->E, T_nodes_dev,
                       alpha_dev, alpha_count > 1 ? 1 : 0, T_ref, th.p, bad.p);
    HIP_TRY(c, hipGetLastError());
    unsigned long long hflags[2] = {~0ull, 0ull};
    HIP_TRY(c, hipMemcpyAsync(hflags, bad.p, sizeof hflags, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const unsigned long long hb = hflags[0];
    if (hb != ~0ull) {
        double v = 0.0;
        HIP_TRY(c, hipMemcpy(&v, th.p + hb, sizeof(double), hipMemcpyDeviceToHost));
        return c->fail(FH_BAD_ARGUMENT, bad_stretch(who, hb, v));
    }
    c->expansion_n = 0;
    c->expansion_identity = hflags[1] == 0;
    std::swap(c->expansion.p, th.p);
    std::swap(c->expansion.n, th.n);
    c->expansion_n = c->E;
    ++c->expansion_gen;
    c->last_kernel = "k_thermal_stretch";
    return FH_OK;
}

int fh_set_thermal_expansion(fh_ctx* c, const double* T_nodes, const double* alpha, uint64_t alpha_count, double T_ref) {
    const char* who = "fh_set_thermal_expansion";
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    int rc = set_ready(c, who);
    if (rc) return rc;
    if (!T_nodes || !alpha) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null argument");
    if (alpha_count != 1 && alpha_count != c->E) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": alpha_count must be 1 or the number of elements");
    DevBuf<double> T, al;
    HIP_TRY(c, T.alloc((size_t)c->N));
    HIP_TRY(c, al.alloc((size_t)alpha_count));
    HIP_TRY(c, hipMemcpyAsync(T.p, T_nodes, sizeof(double) * c->N, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(al.p, alpha, sizeof(double) * alpha_count, hipMemcpyHostToDevice, c->stream));
    return fh_set_thermal_expansion_dev(c, T.p, al.p, alpha_count, T_ref);   // (waits for the stream before it returns: T and al may go)
}

// f_th = -r(0): the residual's own route at u = 0 (the context's u stays where it is and is not read), negated
int fh_thermal_load_dev(fh_ctx* c, double* out_dev) {
    const char* who = "fh_thermal_load";
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (!c->expansion_n) return c->fail(FH_INVALID_STATE, std::string(who) + ": no element expansion set");
    if (c->op != FH_LINEAR_ELASTIC)
        return c->fail(FH_UNSUPPORTED, std::string(who) + ": the element expansion is a load, f_th = -r(0), for FH_LINEAR_ELASTIC only; the hyperelastic "
                                                          "operators carry it in their residual");
    if (!out_dev) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": out is null");
    const long long n = (long long)c->S() * (long long)c->N;
    HIP_TRY(c, hipMemsetAsync(out_dev, 0, sizeof(double) * (size_t)n, c->stream));
    const bool had_u = c->has_u;
    c->has_u = false;
    const int rc = fh_assemble_vector_dev(c, out_dev, nullptr);
    c->has_u = had_u;
    if (rc) return rc;
    if (n) hipLaunchKernelGGL(k_negate, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, n, out_dev);
    HIP_TRY(c, hipGetLastError());
    return FH_OK;
}

int fh_thermal_load(fh_ctx* c, double* out) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (!out) return c->fail(FH_BAD_ARGUMENT, "fh_thermal_load: out is null");
    DevBuf<double> d;
    const size_t n = (size_t)c->S() * c->N;
    HIP_TRY(c, d.alloc(n));
    const int rc = fh_thermal_load_dev(c, d.p);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(out, d.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FH_OK;
}

int fh_element_expansion(fh_ctx* c, double* theta_out) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    if (!c->expansion_n) return c->fail(FH_INVALID_STATE, "fh_element_expansion: no element expansion set");
    if (!theta_out) return c->fail(FH_BAD_ARGUMENT, "fh_element_expansion: null argument");
    if (c->expansion_n == 1) {
        double v = 1.0;
        HIP_TRY(c, hipMemcpyAsync(&v, c->expansion.p, sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        std::fill(theta_out, theta_out + c->E, v);
        return FH_OK;
    }
    HIP_TRY(c, hipMemcpyAsync(theta_out, c->expansion.p, sizeof(double) * c->E, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FH_OK;
}

}  // extern "C"
