// Penalty contact with rigid obstacles, fixed or translating along a path (contact_kernels.hpp holds the arithmetic and the node kernels): the obstacle table of the
// context, the stand-alone launches the routes off the tiles compose, and the C ABI.  Coulomb friction (fh_set_friction) rides in the same table: the
// same kernels add q beside g and H beside B while its flag is set, on the tiles and off them, with no launch of its own.
//
// Where the term enters ("Penalty contact"): on the element tiles it is FUSED into the node pass that finishes the node sums
// (k_operator_from_partials, k_newton_from_partials, k_dynamics_from_partials, k_first_order_from_partials take the table by value and call
// contact_apply / contact_force for the node they already visit: no launch, no pass over memory of its own).  Off the tiles (the quadratic
// and cubic kinds, rule-set tables) the residual and the map are accumulated into a vector anyway, and ONE stand-alone launch adds the term
// to it before the pass that finishes it (k_contact_force behind the node sums of r(u); k_contact_apply before k_mf_finish /
// k_mf_shift_combine; k_contact_diagonal behind the diagonal's sums, once per solve).  Nothing here waits for the device except the energy,
// which hands one double back; nothing uses atomics; the energy partials are summed in a fixed order.
//
// Moving obstacles (fh_set_obstacle_paths, fh_set_obstacle_time): the context keeps the obstacles where fh_set_obstacles put them, the knots
// of their paths and a clock of two times; the offsets d_o(t) and d_o(t_lag) are evaluated on the host when the clock moves, and every
// table built here carries p + d_o(t) and c_o = d_o(t) - d_o(t_lag).  No kernel knows a time.
#include "engine_internal.hpp"

#include <cmath>
#include <cstddef>
#include <cstring>

// (`grid` sits in the four bytes the compiler left before `stiffness`: binaries built against the struct without it stay valid)
static_assert(sizeof(fh_obstacle) == 72 && offsetof(fh_obstacle, stiffness) == 8, "fh_obstacle: the layout of ABI version 1 moved");

namespace {

// (fh_set_mesh* refuses 2^31 vertices or more, so a node index and the number of workgroups fit an int; the kernels index with size_t)
int blocks_of(long long n) { return (int)std::max<long long>(1, (n + 255) / 256); }

// the table of the stand-alone terms: the obstacles as they are set, whatever the scope
ContactTable table_at_u(const fh_ctx* c) {
    ContactTable t = c->contact;
    t.dim = c->ei.d;
    t.X = c->verts.p;
    t.u = c->has_u ? c->u.p : nullptr;
    t.w = c->contact_has_w ? c->contact_w.p : nullptr;
    for (int o = 0; o < t.count; ++o)
        for (int a = 0; a < 3; ++a) {
            const double cur = c->contact_shift[o][a], lag = c->contact_shift_lag[o][a];
            if (cur != 0.0) t.o[o].p[a] += cur;   // (the bits of an obstacle placed at point + d_o(t))
            t.o[o].c[a] = cur - lag;
        }
    t.mult = c->contact_has_mult ? c->contact_mult.p : nullptr;
    t.mult_stride = (size_t)c->N;
    t.friction = t.friction && !c->friction_suspended;
    t.ubar = nullptr;
    t.slip_v = nullptr;
    if (t.friction) {
        t.ubar = c->friction_ubar.p;
        if (c->friction_slip_v) {   // (a central-difference launch)
            t.slip_v = c->friction_slip_v;
            t.slip_dt = c->friction_slip_dt;
            t.eps = c->friction_slip_eps;
        }
    }
    return t;
}

void friction_clear(fh_ctx* c) {
    if (c->friction_set) ++c->friction_gen;
    c->friction_set = false;
    c->contact.friction = 0;
    for (double& m : c->contact.mu) m = 0.0;
}

// (the multipliers belong to the obstacle list and the mesh; the buffer stays for the next ones)
void multipliers_clear(fh_ctx* c) {
    if (c->contact_has_mult) ++c->contact_gen;
    c->contact_has_mult = false;
}

void paths_clear(fh_ctx* c) {
    c->path_begin.clear();
    c->path_time.clear();
    c->path_offset.clear();
    c->contact_t = c->contact_t_lag = 0.0;
    for (int o = 0; o < FH_MAX_OBSTACLES; ++o)
        for (int a = 0; a < 3; ++a) c->contact_shift[o][a] = c->contact_shift_lag[o][a] = 0.0;
}

// d_o(t): piecewise linear through the obstacle's knots, constant before the first and after the last; no knots: zero
void path_offset_at(const fh_ctx* c, int o, double t, double (&d)[3]) {
    d[0] = d[1] = d[2] = 0.0;
    if (c->path_begin.empty()) return;
    const uint64_t b = c->path_begin[(size_t)o], e = c->path_begin[(size_t)o + 1];
    if (b == e) return;
    const double* T = c->path_time.data();
    const double* O = c->path_offset.data();
    uint64_t k;
    if (!(t > T[b])) k = b;
    else if (!(t < T[e - 1])) k = e - 1;
    else {
        k = b;
        while (T[k + 1] <= t) ++k;   // (T[k] <= t < T[k + 1], k + 1 <= e - 1)
        const double w = (t - T[k]) / (T[k + 1] - T[k]);
        for (int a = 0; a < 3; ++a) d[a] = std::fma(w, O[3 * (k + 1) + a] - O[3 * k + a], O[3 * k + a]);
        return;
    }
    for (int a = 0; a < 3; ++a) d[a] = O[3 * k + a];
}

template <class F>
int by_dim(fh_ctx* c, F&& f) {
    return dispatch_or_last(int_list<2, 3>{}, c->ei.d, [&](auto d) {
        f(d);
        return 0;
    });
}

int standalone_ready(fh_ctx* c, const char* who) {
    if (!c->has_mesh || c->ragged) return c->fail(FH_INVALID_STATE, std::string(who) + ": no finite element mesh set");
    if (c->ei.d != 2 && c->ei.d != 3) return c->fail(FH_UNSUPPORTED, std::string(who) + ": the geometric dim must be 2 or 3");
    if (c->has_u && c->S() != c->ei.d)
        return c->fail(FH_UNSUPPORTED, std::string(who) + ": the contact term needs the operator's solution dim to equal the geometric dim");
    return FH_OK;
}

}  // namespace

ContactTable contact_table(const fh_ctx* c) {
    if (c->contact.count == 0 || c->mf_scope != MF_TANGENT) return contact_off();
    return table_at_u(c);
}

int contact_blocked(fh_ctx* c, const char* who) {
    if (c->contact.count && c->op >= 0 && c->S() != c->ei.d)
        return c->fail(FH_UNSUPPORTED, std::string(who) + ": obstacles are set (fh_set_obstacles) and the operator's solution dim is not the geometric dim");
    return FH_OK;
}

// (what contact_table(c).friction says, without forming the table)
bool friction_active(const fh_ctx* c) { return c->contact.count && c->mf_scope == MF_TANGENT && c->contact.friction && !c->friction_suspended; }

// the entries of the lag displacement: one per dof of the mesh (the contact term needs the solution dim to be the geometric one)
static size_t lag_entries(const fh_ctx* c) { return (size_t)c->ei.d * (size_t)c->N; }

unsigned long long contact_key(const fh_ctx* c) { return (c->contact_gen + c->friction_gen) | (friction_active(c) ? 1ull << 63 : 0ull); }

int friction_lag_to_u(fh_ctx* c, double eps) {
    const size_t n = lag_entries(c);
    if (c->has_u) HIP_TRY(c, hipMemcpyAsync(c->friction_ubar.p, c->u.p, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
    else HIP_TRY(c, hipMemsetAsync(c->friction_ubar.p, 0, sizeof(double) * n, c->stream));
    c->contact.eps = eps;
    ++c->friction_gen;
    return FH_OK;
}

bool contact_has_paths(const fh_ctx* c) { return !c->path_begin.empty() && c->path_begin.back() > 0; }

void contact_set_time(fh_ctx* c, double t, double t_lag) {
    c->contact_t = t;
    c->contact_t_lag = t_lag;
    if (!contact_has_paths(c)) return;
    bool moved = false;
    for (int o = 0; o < c->contact.count; ++o) {
        double cur[3], lag[3];
        path_offset_at(c, o, t, cur);
        path_offset_at(c, o, t_lag, lag);
        moved = moved || std::memcmp(cur, c->contact_shift[o], sizeof cur) != 0 || std::memcmp(lag, c->contact_shift_lag[o], sizeof lag) != 0;
        std::copy(cur, cur + 3, c->contact_shift[o]);
        std::copy(lag, lag + 3, c->contact_shift_lag[o]);
    }
    if (moved) ++c->contact_gen;
}

void contact_clear(fh_ctx* c) {
    friction_clear(c);
    paths_clear(c);
    multipliers_clear(c);
    if (c->contact.count || c->contact_has_w) ++c->contact_gen;
    c->contact = contact_off();
    c->contact_has_w = false;
    std::fill(c->contact_grid, c->contact_grid + FH_MAX_OBSTACLES, -1);   // (the grids themselves stay: they belong to the context)
}

int contact_add_force(fh_ctx* c, double* out_dev) {
    const ContactTable t = contact_table(c);
    if (!t.count || c->N == 0) return FH_OK;
    by_dim(c, [&](auto d) { hipLaunchKernelGGL((k_contact_force<d()>), dim3(blocks_of((long long)c->N)), dim3(256), 0, c->stream, t, (int)c->N, out_dev, 3); });
    HIP_TRY(c, hipGetLastError());
    return FH_OK;
}

int contact_add_apply(fh_ctx* c, const double* x_dev, const unsigned char* dmask, const unsigned long long* xbits, double* y_dev) {
    const ContactTable t = contact_table(c);
    if (!t.count || c->N == 0) return FH_OK;
    by_dim(c, [&](auto d) {
        hipLaunchKernelGGL((k_contact_apply<d()>), dim3(blocks_of((long long)c->N)), dim3(256), 0, c->stream, t, (int)c->N, x_dev, dmask, xbits, y_dev);
    });
    HIP_TRY(c, hipGetLastError());
    // (behind mf_single, which names the element kernels it ran; with no element to run it names nothing)
    if (c->E == 0 || (c->has_mask && c->num_active == 0)) c->last_kernel = "k_contact_apply";
    else c->last_kernel += " + k_contact_apply";
    return FH_OK;
}

int contact_add_diagonal(fh_ctx* c, double* diag_dev) {
    const ContactTable t = contact_table(c);
    if (!t.count || c->N == 0) return FH_OK;
    by_dim(c, [&](auto d) { hipLaunchKernelGGL((k_contact_diagonal<d()>), dim3(blocks_of((long long)c->N)), dim3(256), 0, c->stream, t, (int)c->N, diag_dev); });
    HIP_TRY(c, hipGetLastError());
    c->last_kernel = "k_contact_diagonal";   // (the diagonal's own passes leave no name: this is the last kernel of the diagonal with B)
    return FH_OK;
}

// E_c of `t` (friction: its friction potential D) added to *energy: per-workgroup partials in a fixed tree, at most 2048 ordered range
// sums, the ordered host sum
static int energy_of(fh_ctx* c, const ContactTable& t, double* energy, bool friction = false) {
    if (!t.count || c->N == 0 || (friction && !t.friction)) return FH_OK;
    const int count = blocks_of((long long)c->N), ranges = std::min(2048, count);
    DevBuf<double>& part = c->contact_part;
    if (part.n < (size_t)count + (size_t)ranges) HIP_TRY(c, part.alloc((size_t)count + (size_t)ranges));
    by_dim(c, [&](auto d) {
        if (friction) hipLaunchKernelGGL((k_friction_potential<d()>), dim3(count), dim3(256), 0, c->stream, t, (int)c->N, part.p);
        else hipLaunchKernelGGL((k_contact_energy<d()>), dim3(count), dim3(256), 0, c->stream, t, (int)c->N, part.p);
    });
    hipLaunchKernelGGL(k_sum_partial_ranges<1>, dim3(ranges), dim3(256), 0, c->stream, part.p, (long long)count, part.p + count);
    HIP_TRY(c, hipGetLastError());
    double e = 0.0;
    const int rc = sum_partials(c, part.p + count, ranges, 1, &e);   // (waits for the device: one double comes back)
    if (rc) return rc;
    *energy += e;
    return FH_OK;
}
int contact_add_energy(fh_ctx* c, double* energy) { return energy_of(c, contact_table(c), energy); }

extern "C" {

int fh_set_obstacles(fh_ctx* c, const fh_obstacle* obstacles, uint64_t count, const double* node_weights) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    const char* who = "fh_set_obstacles";
    if (count > FH_MAX_OBSTACLES) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": more than FH_MAX_OBSTACLES obstacles");
    if (count && !obstacles) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null obstacle list");
    ContactTable t = contact_off();
    int grid_of[FH_MAX_OBSTACLES];
    std::fill(grid_of, grid_of + FH_MAX_OBSTACLES, -1);
    for (uint64_t i = 0; i < count; ++i) {
        const fh_obstacle& o = obstacles[i];
        ContactObstacle& k = t.o[i];
        if (o.kind != FH_OBSTACLE_HALF_SPACE && o.kind != FH_OBSTACLE_BALL && o.kind != FH_OBSTACLE_CAVITY && o.kind != FH_OBSTACLE_GRID)
            return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": unknown obstacle kind");
        if (o.kind == FH_OBSTACLE_GRID) {   // (before anything of the standing list is touched)
            if (o.grid < 0 || o.grid >= FH_MAX_SDF_GRIDS || c->sdf_grid[o.grid].dim == 0)
                return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": a grid obstacle names a grid that is not live (fh_sdf_grid_create)");
            if (c->has_mesh && !c->ragged && (int)c->sdf_grid[o.grid].dim != c->ei.d)
                return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": the dim of a grid is not the geometric dim of the mesh");
            grid_of[i] = o.grid;
        }
        if (!std::isfinite(o.stiffness) || !(o.stiffness > 0.0)) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": the stiffness must be positive and finite");
        double nn = 0.0;
        for (int a = 0; a < 3; ++a) {
            if (!std::isfinite(o.point[a])) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": a point is not finite");
            if (o.kind == FH_OBSTACLE_HALF_SPACE && !std::isfinite(o.normal[a])) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": a normal is not finite");
            k.p[a] = o.point[a];
            nn += o.kind == FH_OBSTACLE_HALF_SPACE ? o.normal[a] * o.normal[a] : 0.0;
        }
        k.kind = o.kind;
        k.k = o.stiffness;
        k.radius = 0.0;
        if (o.kind == FH_OBSTACLE_HALF_SPACE) {
            if (!(nn > 0.0) || !std::isfinite(nn)) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": a half-space needs a normal that is not zero");
            const double len = std::sqrt(nn);
            for (int a = 0; a < 3; ++a) k.n[a] = o.normal[a] / len;
        } else if (o.kind == FH_OBSTACLE_GRID) {   // (normal and radius are not read: n[] carries the spacings, the union the samples)
            const fh_ctx::SdfGrid& g = c->sdf_grid[o.grid];
            k.grid = g.values.p;
            for (int a = 0; a < 3; ++a) k.n[a] = g.h[a];
        } else {
            if (!std::isfinite(o.radius) || !(o.radius > 0.0)) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": the radius must be positive and finite");
            k.radius = o.radius;
        }
    }
    if (count && node_weights) {
        if (!c->has_mesh || c->ragged) return c->fail(FH_INVALID_STATE, std::string(who) + ": no finite element mesh set");
        for (uint64_t i = 0; i < c->N; ++i)
            if (!std::isfinite(node_weights[i]) || node_weights[i] < 0.0)
                return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": a node weight is negative or not finite");
    }
    if (count == 0) {
        contact_clear(c);
        return FH_OK;
    }
    friction_clear(c);   // (the coefficients belong to the obstacle list)
    paths_clear(c);      // (and so do the paths)
    multipliers_clear(c);   // (and the multipliers)
    if (!c->has_mesh || c->ragged) return c->fail(FH_INVALID_STATE, std::string(who) + ": no finite element mesh set");
    if (c->ei.d != 2 && c->ei.d != 3) return c->fail(FH_UNSUPPORTED, std::string(who) + ": the geometric dim must be 2 or 3");
    if (c->ei.d == 2)   // the third components take no part in a plane problem: a normal is normalised over the first two
        for (uint64_t i = 0; i < count; ++i) {
            ContactObstacle& k = t.o[i];
            if (k.kind != FH_OBSTACLE_HALF_SPACE) continue;
            const double len = std::sqrt(obstacles[i].normal[0] * obstacles[i].normal[0] + obstacles[i].normal[1] * obstacles[i].normal[1]);
            if (!(len > 0.0)) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": a half-space needs a normal that is not zero");
            k.n[0] = obstacles[i].normal[0] / len;
            k.n[1] = obstacles[i].normal[1] / len;
            k.n[2] = 0.0;
        }
    if (node_weights) {
        HIP_TRY(c, c->contact_w.alloc((size_t)c->N + 1));
        HIP_TRY(c, hipMemcpyAsync(c->contact_w.p, node_weights, sizeof(double) * (size_t)c->N, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    t.count = (int)count;
    for (uint64_t i = 0; i < count; ++i) t.grids = t.grids || grid_of[i] >= 0;
    c->contact = t;
    std::copy(grid_of, grid_of + FH_MAX_OBSTACLES, c->contact_grid);
    c->contact_has_w = node_weights != nullptr;
    ++c->contact_gen;
    return FH_OK;
}

int fh_set_obstacle_paths(fh_ctx* c, const uint64_t* knot_begin, const double* knot_time, const double* knot_offset) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    const char* who = "fh_set_obstacle_paths";
    if (!c->contact.count) return c->fail(FH_INVALID_STATE, std::string(who) + ": no obstacles set (fh_set_obstacles)");
    const bool had = contact_has_paths(c);
    if (!knot_begin && !knot_time && !knot_offset) {
        const double t = c->contact_t, t_lag = c->contact_t_lag;
        paths_clear(c);
        c->contact_t = t;
        c->contact_t_lag = t_lag;
        if (had) ++c->contact_gen;
        return FH_OK;
    }
    if (!knot_begin) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null knot_begin");
    const int count = c->contact.count;
    if (knot_begin[0] != 0) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": knot_begin must start at 0");
    for (int o = 0; o < count; ++o)
        if (knot_begin[o + 1] < knot_begin[o]) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": knot_begin must not decrease");
    const uint64_t knots = knot_begin[count];
    if (knots && (!knot_time || !knot_offset)) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null knot_time or knot_offset");
    for (uint64_t k = 0; k < knots; ++k) {
        if (!std::isfinite(knot_time[k])) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": a knot time is not finite");
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(knot_offset[3 * k + a])) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": a knot offset is not finite");
    }
    for (int o = 0; o < count; ++o)
        for (uint64_t k = knot_begin[o]; k + 1 < knot_begin[o + 1]; ++k)
            if (!(knot_time[k + 1] > knot_time[k]))
                return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": the knot times of an obstacle must be strictly increasing");
    c->path_begin.assign(knot_begin, knot_begin + count + 1);
    c->path_time.assign(knot_time, knot_time + knots);
    c->path_offset.assign(knot_offset, knot_offset + 3 * knots);
    if (!contact_has_paths(c)) {   // (no knots at all: as without paths)
        const double t = c->contact_t, t_lag = c->contact_t_lag;
        paths_clear(c);
        c->contact_t = t;
        c->contact_t_lag = t_lag;
        if (had) ++c->contact_gen;
        return FH_OK;
    }
    contact_set_time(c, c->contact_t, c->contact_t_lag);   // the offsets of the clock as it stands
    return FH_OK;
}

int fh_set_obstacle_time(fh_ctx* c, double t, double t_lag) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    const char* who = "fh_set_obstacle_time";
    if (!std::isfinite(t) || !std::isfinite(t_lag)) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": t and t_lag must be finite");
    if (!c->contact.count) return c->fail(FH_INVALID_STATE, std::string(who) + ": no obstacles set (fh_set_obstacles)");
    contact_set_time(c, t, t_lag);
    return FH_OK;
}

int fh_obstacle_count(fh_ctx* c, uint64_t* count) {
    if (!c) return FH_BAD_ARGUMENT;
    if (!count) return c->fail(FH_BAD_ARGUMENT, "fh_obstacle_count: count is null");
    *count = (uint64_t)c->contact.count;
    return FH_OK;
}

int fh_obstacle_offsets(fh_ctx* c, double* current, double* lag) {
    if (!c) return FH_BAD_ARGUMENT;
    if (!c->contact.count) return c->fail(FH_INVALID_STATE, "fh_obstacle_offsets: no obstacles set (fh_set_obstacles)");
    for (int o = 0; o < c->contact.count; ++o)
        for (int a = 0; a < 3; ++a) {
            if (current) current[3 * o + a] = c->contact_shift[o][a];
            if (lag) lag[3 * o + a] = c->contact_shift_lag[o][a];
        }
    return FH_OK;
}

int fh_contact_resultants(fh_ctx* c, double* normal, double* friction) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    const char* who = "fh_contact_resultants";
    if (!normal) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null argument");
    const int rc = standalone_ready(c, who);
    if (rc) return rc;
    const ContactTable t = table_at_u(c);
    std::fill(normal, normal + 3 * t.count, 0.0);
    if (friction) std::fill(friction, friction + 3 * t.count, 0.0);
    if (!t.count || c->N == 0) return FH_OK;
    const int count = blocks_of((long long)c->N), K = 6 * t.count;
    DevBuf<double>& part = c->contact_part;
    if (part.n < (size_t)count * (size_t)K) HIP_TRY(c, part.alloc((size_t)count * (size_t)K));
    by_dim(c, [&](auto d) { hipLaunchKernelGGL((k_contact_resultants<d()>), dim3(count), dim3(256), 0, c->stream, t, (int)c->N, part.p); });
    HIP_TRY(c, hipGetLastError());
    c->last_kernel = "k_contact_resultants";
    std::vector<double> sums((size_t)K);
    const int rs = sum_partials(c, part.p, count, K, sums.data());   // (waits for the device; the rows in index order)
    if (rs) return rs;
    for (int o = 0; o < t.count; ++o)
        for (int a = 0; a < 3; ++a) {
            normal[3 * o + a] = sums[(size_t)(6 * o + a)];
            if (friction) friction[3 * o + a] = sums[(size_t)(6 * o + 3 + a)];
        }
    return FH_OK;
}

int fh_contact_energy(fh_ctx* c, double* energy) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    const char* who = "fh_contact_energy";
    if (!energy) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null argument");
    *energy = 0.0;
    const int rc = standalone_ready(c, who);
    if (rc) return rc;
    c->last_kernel = "k_contact_energy";
    return energy_of(c, table_at_u(c), energy);
}

int fh_contact_force_dev(fh_ctx* c, double* out_dev) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    const char* who = "fh_contact_force_dev";
    if (!out_dev) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null argument");
    const int rc = standalone_ready(c, who);
    if (rc) return rc;
    const ContactTable t = table_at_u(c);
    if (!t.count || c->N == 0) return FH_OK;
    by_dim(c, [&](auto d) { hipLaunchKernelGGL((k_contact_force<d()>), dim3(blocks_of((long long)c->N)), dim3(256), 0, c->stream, t, (int)c->N, out_dev, 1); });
    HIP_TRY(c, hipGetLastError());
    c->last_kernel = "k_contact_force";
    return FH_OK;
}

int fh_set_friction(fh_ctx* c, const double* mu, uint64_t count, double slip_length) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    const char* who = "fh_set_friction";
    if (count == 0 || !mu) {
        friction_clear(c);
        return FH_OK;
    }
    if (!c->contact.count) return c->fail(FH_INVALID_STATE, std::string(who) + ": no obstacles set (fh_set_obstacles)");
    if (count != (uint64_t)c->contact.count) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": count must equal the number of obstacles set");
    if (!std::isfinite(slip_length) || !(slip_length > 0.0)) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": the slip length must be positive and finite");
    bool any = false;
    for (uint64_t i = 0; i < count; ++i) {
        if (!std::isfinite(mu[i]) || mu[i] < 0.0) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": a friction coefficient is negative or not finite");
        any = any || mu[i] > 0.0;
    }
    const size_t n = lag_entries(c);
    if (!c->friction_set) {   // the lag state starts at u = 0
        if (!c->friction_ubar.p || c->friction_ubar.n < n) HIP_TRY(c, c->friction_ubar.alloc(n));
        HIP_TRY(c, hipMemsetAsync(c->friction_ubar.p, 0, sizeof(double) * n, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    for (int i = 0; i < FH_MAX_OBSTACLES; ++i) c->contact.mu[i] = (uint64_t)i < count ? mu[i] + 0.0 : 0.0;
    c->contact.eps = slip_length;
    c->contact.friction = any ? 1 : 0;
    c->friction_set = true;
    ++c->friction_gen;
    return FH_OK;
}

static int friction_reference(fh_ctx* c, const char* who, const double* ubar, hipMemcpyKind kind) {
    if (!c->friction_set) return c->fail(FH_INVALID_STATE, std::string(who) + ": no friction set (fh_set_friction)");
    int rc = standalone_ready(c, who);
    if (rc) return rc;
    if (!ubar) {
        rc = friction_lag_to_u(c, c->contact.eps);
        if (rc) return rc;
    } else {
        HIP_TRY(c, hipMemcpyAsync(c->friction_ubar.p, ubar, sizeof(double) * lag_entries(c), kind, c->stream));
        ++c->friction_gen;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FH_OK;
}
int fh_set_friction_reference(fh_ctx* c, const double* ubar) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    return friction_reference(c, "fh_set_friction_reference", ubar, hipMemcpyHostToDevice);
}
int fh_set_friction_reference_dev(fh_ctx* c, const double* ubar_dev) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    return friction_reference(c, "fh_set_friction_reference_dev", ubar_dev, hipMemcpyDeviceToDevice);
}

int fh_friction_potential(fh_ctx* c, double* potential) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    const char* who = "fh_friction_potential";
    if (!potential) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null argument");
    *potential = 0.0;
    const int rc = standalone_ready(c, who);
    if (rc) return rc;
    c->last_kernel = "k_friction_potential";
    return energy_of(c, table_at_u(c), potential, true);
}

int fh_friction_force_dev(fh_ctx* c, double* out_dev) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    const char* who = "fh_friction_force_dev";
    if (!out_dev) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null argument");
    const int rc = standalone_ready(c, who);
    if (rc) return rc;
    const ContactTable t = table_at_u(c);
    if (!t.friction || c->N == 0) return FH_OK;
    by_dim(c, [&](auto d) { hipLaunchKernelGGL((k_contact_force<d()>), dim3(blocks_of((long long)c->N)), dim3(256), 0, c->stream, t, (int)c->N, out_dev, 2); });
    HIP_TRY(c, hipGetLastError());
    c->last_kernel = "k_contact_force";
    return FH_OK;
}

int fh_contact_gap_dev(fh_ctx* c, double* gap_dev) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    const char* who = "fh_contact_gap_dev";
    if (!gap_dev) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null argument");
    const int rc = standalone_ready(c, who);
    if (rc) return rc;
    if (c->N == 0) return FH_OK;
    const ContactTable t = table_at_u(c);
    by_dim(c, [&](auto d) { hipLaunchKernelGGL((k_contact_gap<d()>), dim3(blocks_of((long long)c->N)), dim3(256), 0, c->stream, t, (int)c->N, gap_dev); });
    HIP_TRY(c, hipGetLastError());
    c->last_kernel = "k_contact_gap";
    return FH_OK;
}

int fh_add_contact_tangent_csr_dev(fh_ctx* c, double* values_dev) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    const char* who = "fh_add_contact_tangent_csr_dev";
    if (!values_dev) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null argument");
    int rc = standalone_ready(c, who);
    if (rc) return rc;
    if (!c->has_pattern) return c->fail(FH_INVALID_STATE, std::string(who) + ": call fh_pattern first");
    if (c->S() != c->ei.d)
        return c->fail(FH_UNSUPPORTED, std::string(who) + ": the contact term needs the operator's solution dim to equal the geometric dim");
    const ContactTable t = table_at_u(c);
    if (!t.count || c->N == 0) return FH_OK;
    by_dim(c, [&](auto d) {
        hipLaunchKernelGGL((k_contact_csr<d()>), dim3(blocks_of((long long)c->N)), dim3(256), 0, c->stream, t, (int)c->N, c->noff.p, c->ncols.p, values_dev);
    });
    HIP_TRY(c, hipGetLastError());
    c->last_kernel = "k_contact_csr";
    return FH_OK;
}

// ---- augmented Lagrangian: the multipliers

static size_t mult_entries(const fh_ctx* c) { return (size_t)c->contact.count * (size_t)c->N; }

static int multipliers_ready(fh_ctx* c, const char* who) {
    if (!c->contact.count) return c->fail(FH_INVALID_STATE, std::string(who) + ": no obstacles set (fh_set_obstacles)");
    return standalone_ready(c, who);
}

// the buffer of the multipliers, count x N doubles; `zero`: filled with zeros (queued on the stream)
static int multipliers_alloc(fh_ctx* c, bool zero) {
    const size_t n = mult_entries(c);
    if (!c->contact_mult.p || c->contact_mult.n < n) HIP_TRY(c, c->contact_mult.alloc(n));
    if (zero && n) HIP_TRY(c, hipMemsetAsync(c->contact_mult.p, 0, sizeof(double) * n, c->stream));
    return FH_OK;
}

static int set_multipliers(fh_ctx* c, const char* who, const double* s, hipMemcpyKind kind) {
    if (!s) {   // clear: back to the instantiations without multipliers
        multipliers_clear(c);
        return FH_OK;
    }
    int rc = multipliers_ready(c, who);
    if (rc) return rc;
    const size_t n = mult_entries(c);
    if (kind == hipMemcpyHostToDevice)
        for (size_t i = 0; i < n; ++i)
            if (!std::isfinite(s[i]) || s[i] < 0.0) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": a multiplier is negative or not finite");
    rc = multipliers_alloc(c, false);
    if (rc) return rc;
    if (n) HIP_TRY(c, hipMemcpyAsync(c->contact_mult.p, s, sizeof(double) * n, kind, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->contact_has_mult = true;
    ++c->contact_gen;
    return FH_OK;
}
int fh_set_contact_multipliers(fh_ctx* c, const double* s) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    return set_multipliers(c, "fh_set_contact_multipliers", s, hipMemcpyHostToDevice);
}
int fh_set_contact_multipliers_dev(fh_ctx* c, const double* s_dev) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    return set_multipliers(c, "fh_set_contact_multipliers_dev", s_dev, hipMemcpyDeviceToDevice);
}

static int get_multipliers(fh_ctx* c, const char* who, double* s, hipMemcpyKind kind) {
    if (!s) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null argument");
    const int rc = multipliers_ready(c, who);
    if (rc) return rc;
    const size_t n = mult_entries(c);
    if (!n) return FH_OK;
    if (c->contact_has_mult) HIP_TRY(c, hipMemcpyAsync(s, c->contact_mult.p, sizeof(double) * n, kind, c->stream));
    else if (kind == hipMemcpyDeviceToDevice) HIP_TRY(c, hipMemsetAsync(s, 0, sizeof(double) * n, c->stream));
    else std::fill(s, s + n, 0.0);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return FH_OK;
}
int fh_contact_multipliers(fh_ctx* c, double* s) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    return get_multipliers(c, "fh_contact_multipliers", s, hipMemcpyDeviceToHost);
}
int fh_contact_multipliers_dev(fh_ctx* c, double* s_dev) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    return get_multipliers(c, "fh_contact_multipliers_dev", s_dev, hipMemcpyDeviceToDevice);
}

int fh_contact_multiplier_forces_dev(fh_ctx* c, double* lam_dev) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    const char* who = "fh_contact_multiplier_forces_dev";
    if (!lam_dev) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null argument");
    const int rc = multipliers_ready(c, who);
    if (rc) return rc;
    if (c->N == 0) return FH_OK;
    const ContactTable t = table_at_u(c);
    by_dim(c, [&](auto d) {
        hipLaunchKernelGGL((k_contact_multiplier_forces<d()>), dim3(blocks_of((long long)c->N)), dim3(256), 0, c->stream, t, (int)c->N, lam_dev);
    });
    HIP_TRY(c, hipGetLastError());
    c->last_kernel = "k_contact_multiplier_forces";
    return FH_OK;
}

int fh_contact_multiplier_update(fh_ctx* c, const uint64_t* skip_nodes, uint64_t skip_count, fh_multiplier_update* stats) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    const char* who = "fh_contact_multiplier_update";
    if (skip_count && !skip_nodes) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null skip_nodes");
    int rc = multipliers_ready(c, who);
    if (rc) return rc;
    for (uint64_t i = 0; i < skip_count; ++i)
        if (skip_nodes[i] >= c->N) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": a skip node is out of range");
    if (stats) *stats = fh_multiplier_update{};
    rc = multipliers_alloc(c, !c->contact_has_mult);   // the first update starts from zeros
    if (rc) return rc;
    c->contact_has_mult = true;
    ++c->contact_gen;
    if (c->N == 0) return FH_OK;
    const unsigned char* skip = nullptr;
    if (skip_count) {
        std::vector<unsigned char> mask((size_t)c->N, 0);
        for (uint64_t i = 0; i < skip_count; ++i) mask[(size_t)skip_nodes[i]] = 1;
        if (c->contact_skip.n < mask.size()) HIP_TRY(c, c->contact_skip.alloc(mask.size()));
        HIP_TRY(c, hipMemcpyAsync(c->contact_skip.p, mask.data(), mask.size(), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));   // (the mask leaves scope)
        skip = c->contact_skip.p;
    }
    ContactTable t = table_at_u(c);
    t.mult = nullptr;   // (the update reads the geometric phi and owns the multipliers it writes)
    const int count = blocks_of((long long)c->N);
    DevBuf<double>& part = c->contact_stat;
    if (part.n < (size_t)count * 4) HIP_TRY(c, part.alloc((size_t)count * 4));
    by_dim(c, [&](auto d) {
        hipLaunchKernelGGL((k_contact_multiplier_update<d()>), dim3(count), dim3(256), 0, c->stream, t, (int)c->N, c->contact_mult.p, (size_t)c->N, skip,
                           part.p);
    });
    HIP_TRY(c, hipGetLastError());
    c->last_kernel = "k_contact_multiplier_update";
    // the rows in index order, as sum_partials takes them (waits for the device)
    std::vector<double> h((size_t)count * 4);
    HIP_TRY(c, hipMemcpyAsync(h.data(), part.p, sizeof(double) * h.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (stats) {
        double active = 0.0;
        for (int b = 0; b < count; ++b) {
            stats->max_change = std::max(stats->max_change, h[(size_t)b * 4]);
            stats->max_penetration = std::max(stats->max_penetration, h[(size_t)b * 4 + 1]);
            active += h[(size_t)b * 4 + 2];
            stats->max_force = std::max(stats->max_force, h[(size_t)b * 4 + 3]);
        }
        stats->active = (uint64_t)active;
    }
    return FH_OK;
}

// ---- sampled signed-distance grids

int fh_sdf_grid_create(fh_ctx* c, uint32_t dim, const uint32_t n[3], const double spacing[3], const double* values, uint32_t* id) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    const char* who = "fh_sdf_grid_create";
    if (!n || !spacing || !values || !id) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null argument");
    if (dim != 2 && dim != 3) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": dim must be 2 or 3");
    if (dim == 2 && n[2] != 1) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": a 2-D grid needs n[2] == 1");
    uint64_t total = 1;
    for (uint32_t a = 0; a < dim; ++a) {
        if (n[a] < 2) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": an axis needs at least 2 samples");
        if (!std::isfinite(spacing[a]) || !(spacing[a] > 0.0)) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": a spacing must be positive and finite");
        total *= n[a];   // (three factors below 2^32: checked after each, no wrap before the test)
        if (total >= (1ull << 31)) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": 2^31 samples or more");
    }
    for (uint64_t i = 0; i < total; ++i)
        if (!std::isfinite(values[i])) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": a sample is not finite");
    int slot = -1;
    for (int s = 0; s < FH_MAX_SDF_GRIDS && slot < 0; ++s)
        if (c->sdf_grid[s].dim == 0) slot = s;
    if (slot < 0) return c->fail(FH_UNSUPPORTED, std::string(who) + ": all FH_MAX_SDF_GRIDS slots are taken");
    fh_ctx::SdfGrid& g = c->sdf_grid[slot];
    // the block: the counts as ints in SDF_GRID_HEADER doubles, then the samples (contact_kernels.hpp)
    const int header[2 * SDF_GRID_HEADER] = {(int)n[0], (int)n[1], dim == 3 ? (int)n[2] : 1, 0};
    static_assert(sizeof header == sizeof(double) * SDF_GRID_HEADER, "the header of a grid block");
    HIP_TRY(c, g.values.alloc((size_t)total + SDF_GRID_HEADER));
    HIP_TRY(c, hipMemcpyAsync(g.values.p, header, sizeof header, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(g.values.p + SDF_GRID_HEADER, values, sizeof(double) * (size_t)total, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int a = 0; a < 3; ++a) {
        g.n[a] = (uint32_t)a < dim ? n[a] : 1u;
        g.h[a] = (uint32_t)a < dim ? spacing[a] : 1.0;
    }
    g.dim = dim;
    *id = (uint32_t)slot;
    return FH_OK;
}

int fh_sdf_grid_destroy(fh_ctx* c, uint32_t id) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    const char* who = "fh_sdf_grid_destroy";
    if (id >= FH_MAX_SDF_GRIDS || c->sdf_grid[id].dim == 0) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": not a live grid");
    for (int o = 0; o < c->contact.count; ++o)
        if (c->contact_grid[o] == (int)id) return c->fail(FH_INVALID_STATE, std::string(who) + ": an obstacle that stands refers to the grid (fh_set_obstacles)");
    HIP_TRY(c, hipStreamSynchronize(c->stream));   // (a launch that reads the samples may still be in flight)
    c->sdf_grid[id].values.release();
    c->sdf_grid[id].dim = 0;
    return FH_OK;
}

int fh_sdf_grid_info(fh_ctx* c, uint32_t id, uint32_t* dim, uint32_t n[3], double spacing[3]) {
    if (!c) return FH_BAD_ARGUMENT;
    if (id >= FH_MAX_SDF_GRIDS || c->sdf_grid[id].dim == 0) return c->fail(FH_BAD_ARGUMENT, "fh_sdf_grid_info: not a live grid");
    const fh_ctx::SdfGrid& g = c->sdf_grid[id];
    if (dim) *dim = g.dim;
    for (int a = 0; a < 3; ++a) {
        if (n) n[a] = g.n[a];
        if (spacing) spacing[a] = g.h[a];
    }
    return FH_OK;
}

int fh_sdf_grid_sample_dev(fh_ctx* c, uint32_t id, const double origin[3], const double* points_dev, uint64_t m, double* phi_dev, double* grad_dev) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    const char* who = "fh_sdf_grid_sample_dev";
    if (id >= FH_MAX_SDF_GRIDS || c->sdf_grid[id].dim == 0) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": not a live grid");
    if (!origin || (m && (!points_dev || !phi_dev))) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null argument");
    if (m == 0) return FH_OK;
    const fh_ctx::SdfGrid& g = c->sdf_grid[id];
    ContactObstacle ob{};
    ob.kind = FH_OBSTACLE_GRID;
    ob.grid = g.values.p;
    for (int a = 0; a < 3; ++a) {
        ob.p[a] = (uint32_t)a < g.dim ? origin[a] : 0.0;
        ob.n[a] = g.h[a];
    }
    const unsigned blocks = (unsigned)std::min<uint64_t>((m + 255) / 256, 65536);   // (grid-stride beyond)
    if (g.dim == 2) hipLaunchKernelGGL((k_sdf_grid_sample<2>), dim3(blocks), dim3(256), 0, c->stream, ob, points_dev, (unsigned long long)m, phi_dev, grad_dev);
    else hipLaunchKernelGGL((k_sdf_grid_sample<3>), dim3(blocks), dim3(256), 0, c->stream, ob, points_dev, (unsigned long long)m, phi_dev, grad_dev);
    HIP_TRY(c, hipGetLastError());
    c->last_kernel = "k_sdf_grid_sample";
    return FH_OK;
}

}  // extern "C"
