// Time integration on the device: M a + r(u) = lf f with the context's residual r and the mass of fh_set_mass_density, by central
// differences (velocity-Verlet form, row-sum lumped mass), Newmark(beta, gamma) or backward Euler (one Newton solve per step: newton_run
// of engine_newton.hip on alpha = 1, beta = newmark_beta dt^2); and the first-order problem M du/dt + r(u) = lf f on the same handle, by
// Runge-Kutta-Legendre super-steps (one stage: forward Euler; lumped mass) or the theta method (newton_run on alpha = 1, beta = theta dt);
// the handle, the step loops, the records and the C ABI
#include "engine_internal.hpp"

#include "dynamics_kernels.hpp"

#include <cmath>

struct fh_dynamics {
    fh_ctx* c = nullptr;
    fh_dynamics_settings s{};          // (a first-order handle keeps its dt and Newton arguments here; s.scheme is not read then)
    int fo_scheme = -1;                // FH_FO_RKL or FH_FO_THETA; -1: the second-order problem of s.scheme
    double theta = 1.0;
    uint32_t stages = 1;
    bool fresh = true;                 // first order: no step call has checked the state since fh_dynamics_set_state
    unsigned long long topo_gen = 0;   // the context's mesh at creation: fh_set_mesh* invalidates the handle
    int n = 0;                         // S N at creation
    DevBuf<double> v, a, m, f, lf, r, rpart, kep, u_ref, u_prev, work, load;
    std::vector<double> h_lf;
    bool has_f = false;
    uint64_t step = 0;                 // steps taken since fh_dynamics_set_state
    // what m (the first five) and a_n (all six; first order: the rate, kept in v) were formed for: struct_gen (operator, table, mask),
    // topo_gen, geom_gen, density_gen, dirichlet_gen, the u_gen this handle left behind, and the contact_gen of fh_set_obstacles with the friction_gen of fh_set_friction (contact_key)
    unsigned long long m_key[5] = {~0ull, ~0ull, ~0ull, ~0ull, ~0ull};
    unsigned long long a_key[7] = {~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull};
    bool load_changed = true;          // (also: the damping coefficients have changed)
    double eta_m = 0.0, eta_k = 0.0;   // Rayleigh damping C = eta_m M + eta_k T(u) (fh_dynamics_set_damping); (0, 0): every launch as without it
    DevBuf<double> u_ref2;             // implicit schemes with damping: the folded u_ref of the step (k_damping_fold)
    double eps_v = 0.0;                // friction: the slip velocity (fh_dynamics_set_slip_velocity); 0: the context's slip length as it is
    // prescribed motion of the Dirichlet dofs (fh_dynamics_set_boundary_motion): u_n = fma(g_n - g_0, direction, u_0) there, g_n =
    // bm_factor[min(n, count - 1)]; bm_u0 is the u fh_dynamics_set_state gave, kept from the first motion on
    DevBuf<double> bm_dir, bm_u0;
    std::vector<double> bm_factor;     // empty: no motion, the Dirichlet dofs are held
};

namespace {

const char* WHO = "fh_dynamics_step";

bool first_order(const fh_dynamics* d) { return d->fo_scheme >= 0; }
// the schemes on the row-sum lumped mass
bool explicit_scheme(const fh_dynamics* d) { return first_order(d) ? d->fo_scheme == FH_FO_RKL : d->s.scheme == FH_DYN_CENTRAL_DIFFERENCE; }
const unsigned char* dmask_of(const fh_ctx* c) { return c->mf_num_dirichlet ? c->mf_dmask.p : nullptr; }
int blocks_of(int n) { return std::max(1, (n + 255) / 256); }

void key_now(const fh_ctx* c, unsigned long long (&k)[7]) {
    k[0] = c->struct_gen;
    k[1] = c->topo_gen;
    k[2] = c->geom_gen;
    k[3] = c->density_gen;
    k[4] = c->dirichlet_gen;
    k[5] = c->u_gen;
    k[6] = contact_key(c);
}

bool boundary_motion(const fh_dynamics* d) { return !d->bm_factor.empty(); }
// g_n - g_0, formed on the host: a pure function of n
double motion_factor(const fh_dynamics* d, uint64_t n) { return d->bm_factor[(size_t)std::min<uint64_t>(n, d->bm_factor.size() - 1)]; }
double motion_offset(const fh_dynamics* d, uint64_t n) { return motion_factor(d, n) - d->bm_factor[0]; }

// the handle still belongs to the context's mesh and the context can form M and r
int dyn_ready(fh_dynamics* d, const char* who) {
    fh_ctx* c = d->c;
    if (c->topo_gen != d->topo_gen || c->S() * (int)c->N != d->n)
        return c->fail(FH_INVALID_STATE, std::string(who) + ": the context's mesh or operator has changed since fh_dynamics_create");
    return mf_shift_ready(c, who, 1.0, 1.0);
}

// the residual's partials over the tiles into d->rpart (*tiles = true), where newton_residual takes the tiles; nothing is waited for
int residual_tiles(fh_dynamics* d, bool* tiles) {
    fh_ctx* c = d->c;
    *tiles = false;
    if (!(c->E > 0 && !c->rs.active)) return FH_OK;
    bool serve;
    const int rc = tile_partials(c, d->rpart, c->S(), &serve);
    if (rc || !serve) return rc;
    // (stiffness damping: r(u) + eta_k T(u) v from one launch of k_damped_pass_tiled; v holds v_h, or v_0 when a_0 is formed)
    const int rt = d->eta_k != 0.0 ? vector_tiles_damped_pass(c->elem_kind, c->op, c->stream, pass_args(c), c->vt.v, active_mask(c), d->v.p, d->eta_k, d->rpart.p)
                                   : vector_tiles_element_pass(c->elem_kind, c->op, c->stream, pass_args(c), c->vt.v, active_mask(c), d->rpart.p);
    if (rt != FH_OK) return FH_OK;
    HIP_TRY(c, hipGetLastError());
    *tiles = true;
    return FH_OK;
}

// r(u) summed into d->r on every other route (newton_residual's second branch): waits for the device and reports the kernels' status;
// with obstacles set, r + g (one launch of k_contact_force behind the node sums)
int residual_summed(fh_dynamics* d) { return ::residual_summed(d->c, d->r.p); }

// y += s T(u) x on the free dofs, T(u) x through tmp: the stiffness part of the damping term on the routes off the tiles and in the implicit
// schemes (tangent_summed, engine_vector.hip: no contact term); waits for the device
int add_tangent(fh_dynamics* d, double s, const double* x, double* tmp, double* y) {
    fh_ctx* c = d->c;
    const int rc = tangent_summed(c, x, tmp);
    if (rc) return rc;
    hipLaunchKernelGGL(k_dynamics_axpy, dim3(blocks_of(d->n)), dim3(256), 0, c->stream, d->n, c->S(), s, dmask_of(c), tmp, y);
    HIP_TRY(c, hipGetLastError());
    return FH_OK;
}

// what the folding of a frozen C into newton_run's arguments cannot express, friction on a first-order handle, and the prescribed
// boundary motions no remedy is chosen for
int damping_supported(fh_dynamics* d, const char* who) {
    fh_ctx* c = d->c;
    if (boundary_motion(d)) {
        if (first_order(d))
            return c->fail(FH_UNSUPPORTED, std::string(who) + ": a boundary motion is set (fh_dynamics_set_boundary_motion) and a first-order handle does not cover it");
        if (d->s.scheme == FH_DYN_NEWMARK)
            return c->fail(FH_UNSUPPORTED, std::string(who) + ": a boundary motion under Newmark is not covered (its kinematics on a prescribed displacement oscillate unless v_0 and a_0 match the path)");
        if (d->s.scheme == FH_DYN_BACKWARD_EULER && (d->eta_m != 0.0 || d->eta_k != 0.0))
            return c->fail(FH_UNSUPPORTED, std::string(who) + ": a boundary motion under backward Euler together with Rayleigh damping is not covered");
    }
    if (first_order(d) && friction_active(c))
        return c->fail(FH_UNSUPPORTED, std::string(who) + ": friction is set (fh_set_friction) and a gradient flow has no slip velocity");
    if (first_order(d) && contact_has_paths(c))
        return c->fail(FH_UNSUPPORTED, std::string(who) + ": an obstacle moves along a path (fh_set_obstacle_paths) and the stage times of a first-order step are not covered");
    if (d->eta_k == 0.0 || explicit_scheme(d)) return FH_OK;
    if (c->op > FH_LINEAR_ELASTIC)
        return c->fail(FH_UNSUPPORTED, std::string(who) + ": stiffness damping under Newmark or backward Euler covers FH_LAPLACE and FH_LINEAR_ELASTIC only");
    if (contact_table(c).count)
        return c->fail(FH_UNSUPPORTED, std::string(who) + ": stiffness damping under Newmark or backward Euler with obstacles set is not covered");
    return FH_OK;
}

// a term of the step takes the velocity the handle holds (Rayleigh damping, friction): a_{n+1} of a step is formed on v_h then, and
// forming it again on v_{n+1} would not repeat it
// ... and so for obstacles on a path: the steps move the contact clock, and contact_gen, themselves
bool velocity_term(const fh_dynamics* d) { return d->eta_m != 0.0 || d->eta_k != 0.0 || friction_active(d->c) || contact_has_paths(d->c); }

// the contact clock of the residual of step `step`: (t_step, t_{step-1}) with t_n = (double)n dt, the records' time column; lagged false
// (a_n of the state as it stands): (t_step, t_step).  Host arithmetic alone; the table of the launch that follows carries the offsets.
void clock_to_step(fh_dynamics* d, uint64_t step, bool lagged) {
    const double t = (double)step * d->s.dt;
    contact_set_time(d->c, t, lagged && step > 0 ? (double)(step - 1) * d->s.dt : t);
}

// the slip length of a step with friction: eps_v dt, or the context's own when no slip velocity was given
double slip_eps(const fh_dynamics* d) { return d->eps_v > 0.0 ? d->eps_v * d->s.dt : d->c->contact.eps; }

int sum_blocks(fh_ctx* c, const double* partial, int count, double* out) { return sum_partials(c, partial, count, 1, out); }

// x . y in a fixed order
int dot(fh_dynamics* d, const double* x, const double* y, double* out) {
    fh_ctx* c = d->c;
    const int g = blocks_of(d->n);
    hipLaunchKernelGGL(k_kinetic_partials, dim3(g), dim3(256), 0, c->stream, d->n, x, y, d->kep.p);
    HIP_TRY(c, hipGetLastError());
    return sum_blocks(c, d->kep.p, g, out);
}

// the row-sum lumped mass m = M 1 (no Dirichlet rows take part) for the current mesh, table, mask and density; every free dof must have m > 0
int ensure_lumped(fh_dynamics* d, const char* who) {
    fh_ctx* c = d->c;
    unsigned long long k[7];
    key_now(c, k);
    if (std::equal(k, k + 5, d->m_key)) return FH_OK;
    // (with damping or friction a_n is not formed again for what the handle itself moves -- remember_u -- and the walk below moves struct_gen on a
    // rule-set table: an a_n that is current on entry stays current)
    const bool a_current = velocity_term(d) && std::equal(k, k + 7, d->a_key) && !d->load_changed;
    const int n = d->n;
    const std::vector<double> ones((size_t)n, 1.0);
    std::vector<double> h((size_t)n);
    HIP_TRY(c, hipMemcpyAsync(d->work.p, ones.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    int rc = mass_full(c, d->work.p, nullptr, d->m.p);
    if (rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(h.data(), d->m.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    std::vector<unsigned char> hm(c->N, 0);
    if (c->mf_num_dirichlet) HIP_TRY(c, hipMemcpyAsync(hm.data(), c->mf_dmask.p, (size_t)c->N, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const int S = c->S();
    for (int i = 0; i < n; ++i)
        if (!hm[(size_t)(i / S)] && !(h[(size_t)i] > 0.0))
            return c->fail(FH_UNSUPPORTED, std::string(who) + ": the row-sum lumped mass of dof " + std::to_string(i) + " (node " + std::to_string(i / S) +
                                               ") is " + std::to_string(h[(size_t)i]) + ", not positive: the explicit schemes need another lumping on this element kind");
    std::copy(k, k + 5, d->m_key);
    if (a_current) key_now(c, d->a_key);
    return FH_OK;
}

// central differences with stiffness damping: (omega dt)^2 + 2 eta_k omega^2 dt <= 4 for the highest mode (the Jury conditions of the
// step matrix of one mode; eta_m drops out): dt_crit = (2 / omega)(sqrt(1 + xi^2) - xi), xi = eta_k omega / 2.  Each operation rounded once.
double damped_dt_crit(double omega, double eta_k) {
#pragma clang fp contract(off)
    const double xi = eta_k * omega / 2.0;
    const double x2 = xi * xi;
    const double root = std::sqrt(1.0 + x2);
    return (2.0 / omega) * (root - xi);
}

DynStep step_args(fh_dynamics* d, int flags, uint64_t step) {
    fh_ctx* c = d->c;
    DynStep p;
    p.dt = d->s.dt;
    p.half_dt = 0.5 * d->s.dt;
    p.f = d->has_f ? d->f.p : nullptr;
    p.lf = d->h_lf.empty() ? nullptr : d->lf.p;
    p.lf_count = d->h_lf.size();
    p.step = step;
    p.m = d->m.p;
    p.dmask = dmask_of(c);
    p.u = c->u.p;
    p.v = d->v.p;
    p.a = d->a.p;
    p.ke_partial = d->kep.p;
    p.flags = flags;
    p.eta_m = d->eta_m;
    if (boundary_motion(d) && (flags & DYN_ADVANCE)) {   // the drift of this launch: from `step` to step + 1
        p.bm_dir = d->bm_dir.p;
        p.bm_u0 = d->bm_u0.p;
        p.bm_g = motion_offset(d, step + 1);
        p.bm_rate = (motion_factor(d, step + 1) - motion_factor(d, step)) / d->s.dt;
    } else if (boundary_motion(d)) {   // (no drift: the fixed branch only leaves v alone)
        p.bm_dir = d->bm_dir.p;
        p.bm_u0 = d->bm_u0.p;
    }
    return p;
}

// one launch of the central-difference update on the residual at the context's u (flags with DYN_ACCEL), or the first kick and drift alone.
// *ke_count: the partials a DYN_STORE launch leaves.  On the tiles nothing is waited for.
int explicit_launch(fh_dynamics* d, int flags, uint64_t step, uint64_t* stats, int* ke_count) {
    fh_ctx* c = d->c;
    const int S = c->S(), n = d->n;
    const DynStep p = step_args(d, flags, step);
    // friction: the lag state is the u the residual is formed at, the slip dt v of the velocity the handle holds (v_h; v_0 for a_0)
    const FrictionSlip slip(c, (flags & DYN_ACCEL) && friction_active(c) ? d->v.p : nullptr, d->s.dt, slip_eps(d));
    if (flags & DYN_ACCEL) {
        clock_to_step(d, step, (flags & DYN_COMPLETE) != 0);
        bool tiles;
        int rc = residual_tiles(d, &tiles);
        if (rc) return rc;
        ++stats[1];
        if (tiles) {
            HIP_TRY(c, vector_tiles_dynamics_node_pass(c->stream, S, (int)c->N, c->vt.v, d->rpart.p, p, contact_table(c)));
            c->last_kernel = d->eta_k != 0.0 ? "k_damped_pass_tiled + k_dynamics_from_partials" : "k_element_pass_tiled + k_dynamics_from_partials";
            if (ke_count) *ke_count = vector_tiles_operator_partials((int)c->N);
            if (flags & DYN_ADVANCE) ++c->u_gen;
            return FH_OK;
        }
        rc = residual_summed(d);
        if (rc) return rc;
        if (d->eta_k != 0.0) {   // r += eta_k T(u) v
            rc = add_tangent(d, d->eta_k, d->v.p, d->work.p, d->r.p);
            if (rc) return rc;
        }
        c->last_kernel = contact_table(c).count ? "k_residual_elements + k_vector_from_elements_soa + k_contact_force + k_dynamics_update"
                                                : "k_residual_elements + k_vector_from_elements_soa + k_dynamics_update";
    }
    hipLaunchKernelGGL(k_dynamics_update, dim3(blocks_of(n)), dim3(256), 0, c->stream, n, S, d->r.p, p);
    HIP_TRY(c, hipGetLastError());
    if (ke_count) *ke_count = blocks_of(n);
    if (flags & DYN_ADVANCE) ++c->u_gen;
    return FH_OK;
}

double load_factor(const fh_dynamics* d, uint64_t step) {
    return d->h_lf.empty() ? 1.0 : d->h_lf[(size_t)std::min<uint64_t>(step, d->h_lf.size() - 1)];
}

// stored energy (with obstacles set: plus the contact energy E_c) and load potential of the state after `step` steps, into row[1..3]
int record_rest(fh_dynamics* d, uint64_t step, double* row) {
    fh_ctx* c = d->c;
    int rc = fh_assemble_scalar(c, &row[1], nullptr);
    if (rc) return rc;
    rc = contact_add_energy(c, &row[1]);
    if (rc) return rc;
    row[2] = 0.0;
    if (d->has_f) {
        rc = dot(d, d->f.p, c->u.p, &row[2]);
        if (rc) return rc;
        row[2] *= load_factor(d, step);
    }
    row[3] = (double)step * d->s.dt;
    return FH_OK;
}

// a_n for the state as it stands, when anything it depends on has changed since it was formed
int ensure_acceleration(fh_dynamics* d, uint64_t* stats) {
    fh_ctx* c = d->c;
    unsigned long long k[7];
    key_now(c, k);
    if (std::equal(k, k + 7, d->a_key) && !d->load_changed) return FH_OK;
    const int n = d->n, S = c->S(), g = blocks_of(n);
    int rc;
    // (v and a of a Dirichlet dof are zero whatever fh_dynamics_set_state was given; with a boundary motion set v there is the handle's own)
    if (!boundary_motion(d)) {
        hipLaunchKernelGGL(k_dynamics_scale, dim3(g), dim3(256), 0, c->stream, n, S, 1.0, dmask_of(c), d->v.p);
        HIP_TRY(c, hipGetLastError());
    }
    if (explicit_scheme(d)) {
        rc = reset_status(c);
        if (rc) return rc;
        rc = explicit_launch(d, DYN_ACCEL, d->step, stats, nullptr);
        if (rc) return rc;
    } else {   // Newmark: M a_0 = lf_0 f - r(u_0) on the free dofs; backward Euler keeps no a_0 but refuses the same states
        clock_to_step(d, d->step, false);
        if (friction_active(c)) {   // (the lag state of a_0 is u_0 itself: no slip, no friction force)
            rc = friction_lag_to_u(c, slip_eps(d));
            if (rc) return rc;
        }
        rc = residual_summed(d);
        if (rc) return rc;
        ++stats[1];
        hipLaunchKernelGGL(k_dynamics_rhs, dim3(g), dim3(256), 0, c->stream, n, S, d->has_f ? d->f.p : nullptr, d->h_lf.empty() ? nullptr : d->lf.p,
                           (unsigned long long)d->h_lf.size(), (unsigned long long)d->step, dmask_of(c), d->r.p, d->work.p);
        HIP_TRY(c, hipGetLastError());
        if (d->eta_k != 0.0 && d->s.scheme == FH_DYN_NEWMARK) {   // M a_0 = lf_0 f - r(u_0) - C v_0: the stiffness part joins the right-hand side
            rc = add_tangent(d, -d->eta_k, d->v.p, d->r.p, d->work.p);
            if (rc) return rc;
        }
        double b2 = 0.0;   // (an inverted NeoHookean state makes r NaN: reported as such, not as a breakdown of the PCG or of Newton)
        rc = dot(d, d->work.p, d->work.p, &b2);
        if (rc) return rc;
        if (!std::isfinite(b2)) return c->fail(FH_DYNAMICS_NONFINITE, std::string(WHO) + ": the residual of the initial state is not finite");
        HIP_TRY(c, hipMemsetAsync(d->a.p, 0, sizeof(double) * (size_t)n, c->stream));
        if (d->s.scheme == FH_DYN_NEWMARK) {
            uint64_t it = 0;
            const int pre = d->s.preconditioner == FH_PRECOND_MULTIGRID ? (int)FH_PRECOND_JACOBI : d->s.preconditioner;   // (M alone needs no hierarchy)
            rc = cg_solve_free_dev(c, WHO, MF_TANGENT, d->work.p, d->a.p, pre, d->s.linear_rel_tol, d->s.linear_max_iter, &it, 1.0, 0.0);
            stats[3] += it;
            if (rc) return rc;
            if (d->eta_m != 0.0) {   // ... and the mass part leaves the solve: a_0 -= eta_m v_0
                hipLaunchKernelGGL(k_dynamics_axpy, dim3(g), dim3(256), 0, c->stream, n, S, -d->eta_m, dmask_of(c), d->v.p, d->a.p);
                HIP_TRY(c, hipGetLastError());
            }
        }
    }
    key_now(c, k);
    std::copy(k, k + 7, d->a_key);
    d->load_changed = false;
    return FH_OK;
}

// a_n belongs to the state the handle has just left behind.  With damping or friction (velocity_term) a step's a_{n+1} (formed on v_h)
// is not what ensure_acceleration would form again for the same state (on v_{n+1}), so nothing the steps themselves moved may make it stale: the walk over the groups of a
// rule-set table stages every group and moves struct_gen, which without damping only forms the same a_n once more.
void remember_u(fh_dynamics* d) {
    if (velocity_term(d)) key_now(d->c, d->a_key);   // (with friction the implicit steps move the lag state, and friction_gen, themselves)
    else d->a_key[5] = d->c->u_gen;
}

int explicit_steps(fh_dynamics* d, uint64_t num_steps, uint64_t record_every, double* records, uint64_t* done, uint64_t* stats) {
    fh_ctx* c = d->c;
    const uint64_t s0 = d->step;
    int rc = reset_status(c);
    if (rc) return rc;
    rc = explicit_launch(d, DYN_ADVANCE, s0, stats, nullptr);   // the first kick and drift of the call
    if (rc) return rc;
    for (uint64_t j = 0; j < num_steps; ++j) {
        const bool last = j + 1 == num_steps;
        const bool rec = last || (record_every && (j + 1) % record_every == 0);
        int ke_count = 0;
        // (a record needs u_{n+1} for the stored energy and the load potential, so the launch of a record stores and stops; every other
        // launch goes straight on to the next kick and drift)
        rc = explicit_launch(d, DYN_ACCEL | DYN_COMPLETE | (rec ? DYN_STORE : DYN_ADVANCE), s0 + j + 1, stats, rec ? &ke_count : nullptr);
        if (rc) return rc;
        if (!rec) continue;
        double row[4] = {0.0, 0.0, 0.0, 0.0};
        rc = sum_blocks(c, d->kep.p, ke_count, &row[0]);   // the host waits here: once per record
        if (rc) return rc;
        row[0] *= 0.5;
        rc = read_status(c, nullptr);
        if (rc) return rc;
        rc = record_rest(d, s0 + j + 1, row);
        if (rc) return rc;
        if (!std::isfinite(row[0]) || !std::isfinite(row[1]))
            return c->fail(FH_DYNAMICS_NONFINITE, std::string(WHO) + ": the kinetic or stored energy after step " + std::to_string(s0 + j + 1) + " is not finite");
        if (records) std::copy(row, row + 4, records + 4 * stats[4]);
        ++stats[4];
        *done = j + 1;
        d->step = s0 + j + 1;
        remember_u(d);
        if (!last) {
            rc = reset_status(c);
            if (rc) return rc;
            rc = explicit_launch(d, DYN_ADVANCE, d->step, stats, nullptr);
            if (rc) return rc;
        }
    }
    return FH_OK;
}

int implicit_steps(fh_dynamics* d, uint64_t num_steps, uint64_t record_every, double* records, uint64_t* done, uint64_t* stats) {
    fh_ctx* c = d->c;
    const int n = d->n, S = c->S(), g = blocks_of(n);
    const bool euler = d->s.scheme == FH_DYN_BACKWARD_EULER;
    const double dt = d->s.dt, nb = euler ? 1.0 : d->s.newmark_beta, bdt2 = nb * dt * dt;
    for (uint64_t j = 0; j < num_steps; ++j) {
        const uint64_t g_step = d->step + 1;
        const double t_before = c->contact_t, t_lag_before = c->contact_t_lag;
        struct ClockBack {   // a step that does not complete, for whatever reason, leaves the clock of the state that stands
            fh_ctx* c;
            double t, t_lag;
            bool armed;
            ~ClockBack() {
                if (armed) contact_set_time(c, t, t_lag);
            }
        } clock_back{c, t_before, t_lag_before, true};
        clock_to_step(d, g_step, true);
        if (friction_active(c)) {   // the lag state of the step is u_n: a device copy enqueued with the step
            const int rf = friction_lag_to_u(c, slip_eps(d));
            if (rf) return rf;
        }
        hipLaunchKernelGGL(k_newmark_predict, dim3(g), dim3(256), 0, c->stream, n, S, dt, euler ? 0.0 : dt * dt * (0.5 - nb), dmask_of(c), c->u.p,
                           d->v.p, d->a.p, d->u_ref.p, d->u_prev.p, boundary_motion(d) ? d->bm_dir.p : nullptr, boundary_motion(d) ? d->bm_u0.p : nullptr,
                           boundary_motion(d) ? motion_offset(d, g_step) : 0.0);
        HIP_TRY(c, hipGetLastError());
        ++c->u_gen;
        const double* load = nullptr;
        if (d->has_f) {   // the load of the step: lf_{n+1} f
            HIP_TRY(c, hipMemcpyAsync(d->load.p, d->f.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
            hipLaunchKernelGGL(k_dynamics_scale, dim3(g), dim3(256), 0, c->stream, n, S, load_factor(d, g_step), (const unsigned char*)nullptr, d->load.p);
            HIP_TRY(c, hipGetLastError());
            load = d->load.p;
        }
        // Rayleigh damping, C frozen at the start of the step, folded into the four arguments (k_damping_fold; the corrector below takes
        // the unmodified u_ref)
        double alpha = 1.0, beta2 = bdt2;
        const double* u_ref = d->u_ref.p;
        int rc;
        if (d->eta_m != 0.0 || d->eta_k != 0.0) {
            const double gdt = (euler ? 1.0 : d->s.newmark_gamma) * dt;
            alpha = 1.0 + d->eta_m * gdt;
            beta2 = bdt2 + d->eta_k * gdt;
            hipLaunchKernelGGL(k_damping_fold, dim3(g), dim3(256), 0, c->stream, n, S, euler ? 0.0 : dt - gdt, d->eta_m * bdt2 / alpha, bdt2, gdt, dmask_of(c),
                               d->u_ref.p, d->v.p, d->a.p, d->u_ref2.p, d->work.p);
            HIP_TRY(c, hipGetLastError());
            u_ref = d->u_ref2.p;
            if (d->eta_k != 0.0) {   // one application of the linear operator, on w
                rc = tangent_summed(c, d->work.p, d->r.p);
                if (rc) return rc;
                hipLaunchKernelGGL(k_damping_load, dim3(g), dim3(256), 0, c->stream, n, bdt2 * load_factor(d, g_step), d->has_f ? d->f.p : nullptr, d->eta_k,
                                   d->r.p, beta2, d->load.p);
                HIP_TRY(c, hipGetLastError());
                load = d->load.p;
            }
        }
        uint64_t st[4] = {0, 0, 0, 0};
        double nm[3] = {0.0, 0.0, 0.0};
        rc = newton_run(c, alpha, beta2, load, u_ref, d->s.newton_tolerance, d->s.newton_max_iterations, d->s.line_search, d->s.preconditioner,
                            d->s.linear_rel_tol, d->s.linear_max_iter, st, nm);
        stats[1] += st[1];
        stats[2] += st[0];
        stats[3] += st[2];
        if (rc) {   // the state stays that of the last completed step
            const std::string msg = c->err;
            HIP_TRY(c, hipMemcpyAsync(c->u.p, d->u_prev.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            ++c->u_gen;
            contact_set_time(c, t_before, t_lag_before);
            remember_u(d);
            return c->fail(rc, msg);
        }
        hipLaunchKernelGGL(k_newmark_correct, dim3(g), dim3(256), 0, c->stream, n, S, euler ? 1 : 0, dt, 1.0 / bdt2, d->s.newmark_gamma, dmask_of(c),
                           c->u.p, d->u_ref.p, d->u_prev.p, d->v.p, d->a.p, boundary_motion(d) ? 1 : 0);
        HIP_TRY(c, hipGetLastError());
        d->step = g_step;
        clock_back.armed = false;
        remember_u(d);
        *done = j + 1;
        const bool last = j + 1 == num_steps;
        if (!(last || (record_every && (j + 1) % record_every == 0))) continue;
        double row[4] = {0.0, 0.0, 0.0, 0.0};
        rc = mass_full(c, d->v.p, nullptr, d->work.p);   // the consistent kinetic energy 1/2 v . M v
        if (rc) return rc;
        rc = dot(d, d->v.p, d->work.p, &row[0]);
        if (rc) return rc;
        row[0] *= 0.5;
        rc = record_rest(d, g_step, row);
        if (rc) return rc;
        if (records) std::copy(row, row + 4, records + 4 * stats[4]);
        ++stats[4];
        if (!std::isfinite(row[0]) || !std::isfinite(row[1]))
            return c->fail(FH_DYNAMICS_NONFINITE, std::string(WHO) + ": the kinetic or stored energy after step " + std::to_string(g_step) + " is not finite");
    }
    return FH_OK;
}

// ---- first order
FoStage stage_args(fh_dynamics* d, int flags, uint64_t step, double mut_dt, double mu, double nu) {
    fh_ctx* c = d->c;
    FoStage p;
    p.mut_dt = mut_dt;
    p.mu = mu;
    p.nu = nu;
    p.f = d->has_f ? d->f.p : nullptr;
    p.lf = d->h_lf.empty() ? nullptr : d->lf.p;
    p.lf_count = d->h_lf.size();
    p.step = step;
    p.m = d->m.p;
    p.dmask = dmask_of(c);
    p.u = c->u.p;
    p.prev = d->u_prev.p;
    p.rate = d->v.p;
    p.partial = d->kep.p;
    p.flags = flags;
    return p;
}

// one stage (or the rate, FO_RATE) on the residual at the context's u.  *count: the partials a FO_STORE launch leaves.  On the tiles
// nothing is waited for.
int first_order_launch(fh_dynamics* d, const FoStage& p, uint64_t* stats, int* count) {
    fh_ctx* c = d->c;
    const int S = c->S(), n = d->n;
    bool tiles;
    int rc = residual_tiles(d, &tiles);
    if (rc) return rc;
    ++stats[1];
    if (tiles) {
        HIP_TRY(c, vector_tiles_first_order_node_pass(c->stream, S, (int)c->N, c->vt.v, d->rpart.p, p, contact_table(c)));
        c->last_kernel = "k_element_pass_tiled + k_first_order_from_partials";
        if (count) *count = vector_tiles_operator_partials((int)c->N);
    } else {
        rc = residual_summed(d);
        if (rc) return rc;
        hipLaunchKernelGGL(k_first_order_update, dim3(blocks_of(n)), dim3(256), 0, c->stream, n, S, d->r.p, p);
        HIP_TRY(c, hipGetLastError());
        c->last_kernel = contact_table(c).count ? "k_residual_elements + k_vector_from_elements_soa + k_contact_force + k_first_order_update"
                                                : "k_residual_elements + k_vector_from_elements_soa + k_first_order_update";
        if (count) *count = blocks_of(n);
    }
    if (!(p.flags & FO_RATE)) ++c->u_gen;
    return FH_OK;
}

// the right-hand side lf_n f - r(u_n) of the state as it stands, refused when it is not finite, and with `solve` the rate du/dt into v
// (RKL: L(u_n), which is that right-hand side over m; theta: M w = lf_n f - r(u_n) on the free dofs by the CG of Newmark's a_0), when
// anything it depends on has changed since it was formed
int ensure_rate(fh_dynamics* d, bool solve, uint64_t* stats) {
    fh_ctx* c = d->c;
    unsigned long long k[7];
    key_now(c, k);
    if (std::equal(k, k + 7, d->a_key) && !d->load_changed) return FH_OK;
    const int n = d->n, S = c->S(), g = blocks_of(n);
    const double* rhs = d->v.p;
    int rc;
    if (d->fo_scheme == FH_FO_RKL) {
        rc = reset_status(c);
        if (rc) return rc;
        rc = first_order_launch(d, stage_args(d, FO_RATE, d->step, 0.0, 0.0, 0.0), stats, nullptr);
        if (rc) return rc;
    } else {
        rc = residual_summed(d);
        if (rc) return rc;
        ++stats[1];
        hipLaunchKernelGGL(k_dynamics_rhs, dim3(g), dim3(256), 0, c->stream, n, S, d->has_f ? d->f.p : nullptr, d->h_lf.empty() ? nullptr : d->lf.p,
                           (unsigned long long)d->h_lf.size(), (unsigned long long)d->step, dmask_of(c), d->r.p, d->work.p);
        HIP_TRY(c, hipGetLastError());
        rhs = d->work.p;
    }
    double b2 = 0.0;   // (an inverted NeoHookean state makes r NaN: reported as such, not as a breakdown of the PCG or of Newton)
    rc = dot(d, rhs, rhs, &b2);
    if (rc) return rc;
    if (!std::isfinite(b2)) return c->fail(FH_DYNAMICS_NONFINITE, std::string(WHO) + ": the residual of the initial state is not finite");
    if (d->fo_scheme == FH_FO_RKL) {
        rc = read_status(c, nullptr);
        if (rc) return rc;
    }
    if (d->fo_scheme == FH_FO_THETA) {
        if (!solve) return FH_OK;   // (a step needs the check alone)
        HIP_TRY(c, hipMemsetAsync(d->v.p, 0, sizeof(double) * (size_t)n, c->stream));
        uint64_t it = 0;
        const int pre = d->s.preconditioner == FH_PRECOND_MULTIGRID ? (int)FH_PRECOND_JACOBI : d->s.preconditioner;   // (M alone needs no hierarchy)
        rc = cg_solve_free_dev(c, WHO, MF_TANGENT, d->work.p, d->v.p, pre, d->s.linear_rel_tol, d->s.linear_max_iter, &it, 1.0, 0.0);
        stats[3] += it;
        if (rc) return rc;
    }
    key_now(c, k);
    std::copy(k, k + 7, d->a_key);
    d->load_changed = false;
    return FH_OK;
}

// the end of a recorded first-order step: row[0] holds u^T B u; *done and the step counter move only when the record is clean
int first_order_record(fh_dynamics* d, uint64_t g_step, double* row, double* records, uint64_t* stats) {
    fh_ctx* c = d->c;
    row[0] *= 0.5;
    int rc = record_rest(d, g_step, row);
    if (rc) return rc;
    if (!std::isfinite(row[0]) || !std::isfinite(row[1]))
        return c->fail(FH_DYNAMICS_NONFINITE, std::string(WHO) + ": 1/2 u^T B u or the stored energy after step " + std::to_string(g_step) + " is not finite");
    if (records) std::copy(row, row + 4, records + 4 * stats[4]);
    ++stats[4];
    return FH_OK;
}

// Runge-Kutta-Legendre: s stages per step, each the residual's element pass and one node pass; the loop only enqueues between records
int first_order_explicit_steps(fh_dynamics* d, uint64_t num_steps, uint64_t record_every, double* records, uint64_t* done, uint64_t* stats) {
    fh_ctx* c = d->c;
    const uint64_t s0 = d->step;
    const uint32_t s = d->stages;
    const double w1dt = 2.0 / ((double)s * (double)s + (double)s) * d->s.dt;
    int rc = reset_status(c);
    if (rc) return rc;
    for (uint64_t j = 0; j < num_steps; ++j) {
        const bool last = j + 1 == num_steps;
        const bool rec = last || (record_every && (j + 1) % record_every == 0);
        int count = 0;
        for (uint32_t k = 1; k <= s; ++k) {
            const double mu = (2.0 * k - 1.0) / k, nu = (1.0 - k) / k;
            const int flags = (k == 1 ? FO_FIRST : 0) | (k < s ? FO_KEEP : 0) | (k == s && rec ? FO_STORE : 0);
            rc = first_order_launch(d, stage_args(d, flags, s0 + j, k == 1 ? w1dt : mu * w1dt, mu, nu), stats, &count);
            if (rc) return rc;
        }
        if (!rec) continue;
        double row[4] = {0.0, 0.0, 0.0, 0.0};
        rc = sum_blocks(c, d->kep.p, count, &row[0]);   // the host waits here: once per record
        if (rc) return rc;
        rc = read_status(c, nullptr);
        if (rc) return rc;
        rc = first_order_record(d, s0 + j + 1, row, records, stats);
        if (rc) return rc;
        *done = j + 1;
        d->step = s0 + j + 1;
        if (!last) {
            rc = reset_status(c);
            if (rc) return rc;
        }
    }
    return FH_OK;
}

// theta method: one newton_run per step on alpha = 1, beta = theta dt, u_ref = u_n, from the guess u_n
int first_order_theta_steps(fh_dynamics* d, uint64_t num_steps, uint64_t record_every, double* records, uint64_t* done, uint64_t* stats) {
    fh_ctx* c = d->c;
    const int n = d->n, g = blocks_of(n);
    const double dt = d->s.dt, cw = (1.0 - d->theta) / d->theta;
    for (uint64_t j = 0; j < num_steps; ++j) {
        const uint64_t g_step = d->step + 1;
        HIP_TRY(c, hipMemcpyAsync(d->u_prev.p, c->u.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
        int rc;
        if (cw != 0.0) {
            rc = residual_summed(d);
            if (rc) return rc;
            ++stats[1];
        }
        const double* load = nullptr;
        if (d->has_f || cw != 0.0) {
            hipLaunchKernelGGL(k_theta_load, dim3(g), dim3(256), 0, c->stream, n, d->has_f ? d->f.p : nullptr, d->h_lf.empty() ? nullptr : d->lf.p,
                               (unsigned long long)d->h_lf.size(), (unsigned long long)d->step, cw, d->r.p, d->load.p);
            HIP_TRY(c, hipGetLastError());
            load = d->load.p;
        }
        uint64_t st[4] = {0, 0, 0, 0};
        double nm[3] = {0.0, 0.0, 0.0};
        rc = newton_run(c, 1.0, d->theta * dt, load, d->u_prev.p, d->s.newton_tolerance, d->s.newton_max_iterations, d->s.line_search,
                        d->s.preconditioner, d->s.linear_rel_tol, d->s.linear_max_iter, st, nm);
        stats[1] += st[1];
        stats[2] += st[0];
        stats[3] += st[2];
        if (rc) {   // the state stays that of the last completed step
            const std::string msg = c->err;
            HIP_TRY(c, hipMemcpyAsync(c->u.p, d->u_prev.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            ++c->u_gen;
            return c->fail(rc, msg);
        }
        d->step = g_step;
        *done = j + 1;
        const bool last = j + 1 == num_steps;
        if (!(last || (record_every && (j + 1) % record_every == 0))) continue;
        double row[4] = {0.0, 0.0, 0.0, 0.0};
        rc = mass_full(c, c->u.p, nullptr, d->work.p);   // u^T M u with the consistent mass
        if (rc) return rc;
        rc = dot(d, c->u.p, d->work.p, &row[0]);
        if (rc) return rc;
        rc = first_order_record(d, g_step, row, records, stats);
        if (rc) return rc;
    }
    return FH_OK;
}

int set_state_common(fh_dynamics* d, const double* u, const double* v, hipMemcpyKind kind) {
    fh_ctx* c = d->c;
    if (first_order(d) && v) return c->fail(FH_BAD_ARGUMENT, "fh_dynamics_set_state: the state of a first-order handle is u alone: v must be null");
    int rc = dyn_ready(d, "fh_dynamics_set_state");
    if (rc) return rc;
    const size_t bytes = sizeof(double) * (size_t)d->n;
    if (u) {
        rc = kind == hipMemcpyHostToDevice ? fh_set_u(c, u) : fh_set_u_dev(c, u);
    } else {
        std::vector<double> z((size_t)d->n, 0.0);
        rc = fh_set_u(c, z.data());
    }
    if (rc) return rc;
    if (v) HIP_TRY(c, hipMemcpyAsync(d->v.p, v, bytes, kind, c->stream));
    else HIP_TRY(c, hipMemsetAsync(d->v.p, 0, bytes, c->stream));
    HIP_TRY(c, hipMemsetAsync(d->a.p, 0, bytes, c->stream));
    if (d->bm_u0.p && d->n) HIP_TRY(c, hipMemcpyAsync(d->bm_u0.p, c->u.p, bytes, hipMemcpyDeviceToDevice, c->stream));   // u_0 of a boundary motion
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    d->step = 0;
    d->a_key[5] = ~0ull;
    d->fresh = true;
    contact_set_time(c, 0.0, 0.0);
    return FH_OK;
}

int set_load_common(fh_dynamics* d, const double* f, const double* load_factor, uint64_t count, hipMemcpyKind kind) {
    fh_ctx* c = d->c;
    if (load_factor && count == 0) return c->fail(FH_BAD_ARGUMENT, "fh_dynamics_set_load: load_factor needs count >= 1");
    d->has_f = f != nullptr;
    if (f) HIP_TRY(c, hipMemcpyAsync(d->f.p, f, sizeof(double) * (size_t)d->n, kind, c->stream));
    d->h_lf.clear();
    if (load_factor) {
        d->h_lf.assign(load_factor, load_factor + count);
        if (d->lf.n < count) HIP_TRY(c, d->lf.alloc((size_t)count));
        HIP_TRY(c, hipMemcpyAsync(d->lf.p, d->h_lf.data(), sizeof(double) * (size_t)count, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    d->load_changed = true;
    return FH_OK;
}

int set_motion_common(fh_dynamics* d, const double* direction, const double* factor, uint64_t count, hipMemcpyKind kind) {
    fh_ctx* c = d->c;
    const char* who = "fh_dynamics_set_boundary_motion";
    if (!direction) {
        if (boundary_motion(d)) d->load_changed = true;   // a_n is formed again, as after fh_dynamics_set_load
        d->bm_factor.clear();
        return FH_OK;
    }
    if (!factor || count == 0) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": the factor table needs count >= 1");
    for (uint64_t k = 0; k < count; ++k)
        if (!std::isfinite(factor[k])) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": a factor is not finite");
    int rc = dyn_ready(d, who);
    if (rc) return rc;
    const size_t n = (size_t)d->n;
    if (d->bm_dir.n < n) HIP_TRY(c, d->bm_dir.alloc(n));
    const bool first = d->bm_u0.n < n || !d->bm_u0.p;
    if (first) {   // u_0: the state as it stands (its Dirichlet entries have not moved since fh_dynamics_set_state), zeros before one
        HIP_TRY(c, d->bm_u0.alloc(n));
        if (c->has_u && n) HIP_TRY(c, hipMemcpyAsync(d->bm_u0.p, c->u.p, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
        else HIP_TRY(c, hipMemsetAsync(d->bm_u0.p, 0, sizeof(double) * std::max<size_t>(n, 1), c->stream));
    }
    if (n) HIP_TRY(c, hipMemcpyAsync(d->bm_dir.p, direction, sizeof(double) * n, kind, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    d->bm_factor.assign(factor, factor + count);
    d->load_changed = true;
    return FH_OK;
}

int state_common(fh_dynamics* d, double* u, double* v, double* a, double* time, uint64_t* step, hipMemcpyKind kind) {
    fh_ctx* c = d->c;
    int rc = dyn_ready(d, "fh_dynamics_state");
    if (rc) return rc;
    const size_t bytes = sizeof(double) * (size_t)d->n;
    if (boundary_motion(d) || (first_order(d) && contact_has_paths(c))) {   // (out of scope whatever is asked for)
        rc = damping_supported(d, "fh_dynamics_state");
        if (rc) return rc;
    }
    if ((first_order(d) ? v : a) && c->has_u && c->N) {   // a_n of the state as it stands (a_0 before the first step); first order: the rate
        uint64_t st[5] = {0, 0, 0, 0, 0};
        rc = damping_supported(d, "fh_dynamics_state");
        if (rc) return rc;
        if (explicit_scheme(d)) rc = ensure_lumped(d, "fh_dynamics_state");
        if (!rc) rc = first_order(d) ? ensure_rate(d, true, st) : ensure_acceleration(d, st);
        if (rc) return rc;
    }
    if (u) {
        if (!c->has_u) return c->fail(FH_INVALID_STATE, "fh_dynamics_state: no state set");
        HIP_TRY(c, hipMemcpyAsync(u, c->u.p, bytes, kind, c->stream));
    }
    if (v) HIP_TRY(c, hipMemcpyAsync(v, d->v.p, bytes, kind, c->stream));
    if (a) HIP_TRY(c, hipMemcpyAsync(a, d->a.p, bytes, kind, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (time) *time = (double)d->step * d->s.dt;
    if (step) *step = d->step;
    return FH_OK;
}

// the handle of either problem: `implicit` checks the Newton arguments of s and takes the vectors of the Newton steps
int create_handle(fh_ctx* c, const char* who, const fh_dynamics_settings& s, bool implicit, int fo_scheme, double theta, uint32_t stages,
                  fh_dynamics** out) {
    if (implicit) {
        if (!std::isfinite(s.newton_tolerance) || !std::isfinite(s.linear_rel_tol))
            return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": the tolerances must be finite");
        if (s.line_search != FH_NEWTON_NO_LINE_SEARCH && s.line_search != FH_NEWTON_BACKTRACKING)
            return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": unknown line search");
        if (s.preconditioner != FH_PRECOND_IDENTITY && s.preconditioner != FH_PRECOND_JACOBI && s.preconditioner != FH_PRECOND_MULTIGRID)
            return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": unknown preconditioner");
    }
    int rc = mf_shift_ready(c, who, 1.0, 1.0);   // FH_UNSUPPORTED: mass operators, FH_TENSOR; FH_INVALID_STATE: no mesh, table or density
    if (rc) return rc;
    fh_dynamics* d = new fh_dynamics;
    d->c = c;
    d->s = s;
    d->fo_scheme = fo_scheme;
    d->theta = theta;
    d->stages = stages;
    d->topo_gen = c->topo_gen;
    d->n = c->S() * (int)c->N;
    const size_t n = (size_t)d->n;
    hipError_t e = hipSuccess;
    auto get = [&](DevBuf<double>& b, size_t count) { if (e == hipSuccess) e = b.alloc(count); };
    get(d->v, n); get(d->a, n); get(d->m, n); get(d->f, n); get(d->r, n); get(d->work, n);
    get(d->kep, (size_t)blocks_of(d->n));
    if (implicit) { get(d->u_prev, n); get(d->load, n); }
    if (implicit && fo_scheme < 0) get(d->u_ref, n);
    if (fo_scheme == FH_FO_RKL && stages > 1) get(d->u_prev, n);   // (Y_{j-2} of the stages)
    if (e == hipSuccess) e = hipMemsetAsync(d->v.p, 0, sizeof(double) * std::max<size_t>(n, 1), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d->a.p, 0, sizeof(double) * std::max<size_t>(n, 1), c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        delete d;
        return e == hipErrorOutOfMemory ? c->fail(FH_OUT_OF_MEMORY, std::string(who) + ": no room for the state vectors") : c->hip_fail(e, who);
    }
    *out = d;
    return FH_OK;
}

}  // namespace

extern "C" {

int fh_dynamics_create(fh_ctx* c, const fh_dynamics_settings* s, fh_dynamics** out) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    const char* who = "fh_dynamics_create";
    if (!s || !out) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null argument");
    *out = nullptr;
    if (s->scheme != FH_DYN_CENTRAL_DIFFERENCE && s->scheme != FH_DYN_BACKWARD_EULER && s->scheme != FH_DYN_NEWMARK)
        return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": unknown scheme");
    if (!std::isfinite(s->dt) || !(s->dt > 0.0)) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": dt must be positive and finite");
    if (s->scheme == FH_DYN_NEWMARK && (!std::isfinite(s->newmark_beta) || !(s->newmark_beta > 0.0) || !std::isfinite(s->newmark_gamma)))
        return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": newmark_beta must be positive and newmark_gamma finite");
    return create_handle(c, who, *s, s->scheme != FH_DYN_CENTRAL_DIFFERENCE, -1, 1.0, 1, out);
}

int fh_first_order_create(fh_ctx* c, const fh_first_order_settings* s, fh_dynamics** out) {
    if (!c) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(c->device);
    const char* who = "fh_first_order_create";
    if (!s || !out) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null argument");
    *out = nullptr;
    if (s->scheme != FH_FO_RKL && s->scheme != FH_FO_THETA) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": unknown scheme");
    if (!std::isfinite(s->dt) || !(s->dt > 0.0)) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": dt must be positive and finite");
    if (s->scheme == FH_FO_RKL && s->stages == 0) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": stages must be at least 1");
    if (s->scheme == FH_FO_THETA && !(s->theta >= 0.5 && s->theta <= 1.0))
        return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": theta must lie in [0.5, 1]");
    fh_dynamics_settings ds{};
    ds.dt = s->dt;
    ds.newton_tolerance = s->newton_tolerance;
    ds.newton_max_iterations = s->newton_max_iterations;
    ds.line_search = s->line_search;
    ds.preconditioner = s->preconditioner;
    ds.linear_rel_tol = s->linear_rel_tol;
    ds.linear_max_iter = s->linear_max_iter;
    return create_handle(c, who, ds, s->scheme == FH_FO_THETA, s->scheme, s->scheme == FH_FO_THETA ? s->theta : 1.0,
                         s->scheme == FH_FO_RKL ? s->stages : 1, out);
}
void fh_dynamics_destroy(fh_dynamics* d) {
    if (!d) return;
    DevGuard dev_guard_(d->c->device);
    delete d;
}

int fh_dynamics_set_state(fh_dynamics* d, const double* u, const double* v) {
    if (!d) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(d->c->device);
    return set_state_common(d, u, v, hipMemcpyHostToDevice);
}
int fh_dynamics_set_state_dev(fh_dynamics* d, const double* u_dev, const double* v_dev) {
    if (!d) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(d->c->device);
    return set_state_common(d, u_dev, v_dev, hipMemcpyDeviceToDevice);
}

int fh_dynamics_set_load(fh_dynamics* d, const double* f, const double* load_factor, uint64_t count) {
    if (!d) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(d->c->device);
    return set_load_common(d, f, load_factor, count, hipMemcpyHostToDevice);
}
int fh_dynamics_set_load_dev(fh_dynamics* d, const double* f_dev, const double* load_factor, uint64_t count) {
    if (!d) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(d->c->device);
    return set_load_common(d, f_dev, load_factor, count, hipMemcpyDeviceToDevice);
}

int fh_dynamics_set_boundary_motion(fh_dynamics* d, const double* direction, const double* factor, uint64_t count) {
    if (!d) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(d->c->device);
    return set_motion_common(d, direction, factor, count, hipMemcpyHostToDevice);
}
int fh_dynamics_set_boundary_motion_dev(fh_dynamics* d, const double* direction_dev, const double* factor, uint64_t count) {
    if (!d) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(d->c->device);
    return set_motion_common(d, direction_dev, factor, count, hipMemcpyDeviceToDevice);
}

int fh_dynamics_set_damping(fh_dynamics* d, double eta_mass, double eta_stiffness) {
    if (!d) return FH_BAD_ARGUMENT;
    fh_ctx* c = d->c;
    DevGuard dev_guard_(c->device);
    const char* who = "fh_dynamics_set_damping";
    if (first_order(d)) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": a first-order problem has no velocity to damp");
    if (!std::isfinite(eta_mass) || !std::isfinite(eta_stiffness) || eta_mass < 0.0 || eta_stiffness < 0.0)
        return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": the coefficients must be finite and not negative");
    if ((eta_mass != 0.0 || eta_stiffness != 0.0) && !explicit_scheme(d) && d->u_ref2.n < (size_t)d->n) HIP_TRY(c, d->u_ref2.alloc((size_t)d->n));
    if (eta_mass != d->eta_m || eta_stiffness != d->eta_k) d->load_changed = true;   // a_n is formed again, as after fh_dynamics_set_load
    d->eta_m = eta_mass + 0.0;   // (-0 -> +0)
    d->eta_k = eta_stiffness + 0.0;
    return FH_OK;
}
int fh_dynamics_set_slip_velocity(fh_dynamics* d, double eps_v) {
    if (!d) return FH_BAD_ARGUMENT;
    fh_ctx* c = d->c;
    const char* who = "fh_dynamics_set_slip_velocity";
    if (first_order(d)) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": a first-order problem has no slip velocity");
    if (!std::isfinite(eps_v) || !(eps_v > 0.0)) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": the slip velocity must be positive and finite");
    if (eps_v != d->eps_v) d->load_changed = true;   // a_n is formed again, as after fh_dynamics_set_load
    d->eps_v = eps_v;
    return FH_OK;
}
int fh_dynamics_damping(fh_dynamics* d, double* eta_mass, double* eta_stiffness) {
    if (!d) return FH_BAD_ARGUMENT;
    if (first_order(d)) return d->c->fail(FH_BAD_ARGUMENT, "fh_dynamics_damping: a first-order problem has no velocity to damp");
    if (eta_mass) *eta_mass = d->eta_m;
    if (eta_stiffness) *eta_stiffness = d->eta_k;
    return FH_OK;
}

int fh_dynamics_step(fh_dynamics* d, uint64_t num_steps, uint64_t record_every, double* records, uint64_t* steps_done, uint64_t* stats) {
    if (!d) return FH_BAD_ARGUMENT;
    fh_ctx* c = d->c;
    DevGuard dev_guard_(c->device);
    uint64_t st[5] = {0, 0, 0, 0, 0}, done = 0;
    if (steps_done) *steps_done = 0;
    if (stats) std::fill(stats, stats + 5, 0);
    int rc = dyn_ready(d, WHO);
    if (rc) return rc;
    if (c->N == 0 || num_steps == 0) return FH_OK;
    if (!c->has_u) {
        rc = set_state_common(d, nullptr, nullptr, hipMemcpyHostToDevice);
        if (rc) return rc;
    }
    rc = damping_supported(d, WHO);
    if (rc) return rc;
    if (explicit_scheme(d)) rc = ensure_lumped(d, WHO);
    if (first_order(d)) {   // (the steps do not read the rate: the state is checked once)
        if (!rc && d->fresh) rc = ensure_rate(d, false, st);
        if (!rc) {
            d->fresh = false;
            rc = explicit_scheme(d) ? first_order_explicit_steps(d, num_steps, record_every, records, &done, st)
                                    : first_order_theta_steps(d, num_steps, record_every, records, &done, st);
        }
    } else {
        if (!rc) rc = ensure_acceleration(d, st);
        if (!rc)
            rc = explicit_scheme(d) ? explicit_steps(d, num_steps, record_every, records, &done, st)
                                    : implicit_steps(d, num_steps, record_every, records, &done, st);
    }
    st[0] = done;
    if (steps_done) *steps_done = done;
    if (stats) std::copy(st, st + 5, stats);
    return rc;
}

int fh_dynamics_state(fh_dynamics* d, double* u, double* v, double* a, double* time, uint64_t* step) {
    if (!d) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(d->c->device);
    return state_common(d, u, v, a, time, step, hipMemcpyDeviceToHost);
}
int fh_dynamics_state_dev(fh_dynamics* d, double* u_dev, double* v_dev, double* a_dev, double* time, uint64_t* step) {
    if (!d) return FH_BAD_ARGUMENT;
    DevGuard dev_guard_(d->c->device);
    return state_common(d, u_dev, v_dev, a_dev, time, step, hipMemcpyDeviceToDevice);
}

int fh_dynamics_stable_dt(fh_dynamics* d, uint32_t iterations, double* omega_max, double* dt_crit) {
    if (!d) return FH_BAD_ARGUMENT;
    fh_ctx* c = d->c;
    DevGuard dev_guard_(c->device);
    const char* who = "fh_dynamics_stable_dt";
    if (!omega_max || !dt_crit || iterations == 0) return c->fail(FH_BAD_ARGUMENT, std::string(who) + ": null result or no iterations");
    int rc = dyn_ready(d, who);
    if (rc) return rc;
    if (!c->has_u) {
        rc = set_state_common(d, nullptr, nullptr, hipMemcpyHostToDevice);
        if (rc) return rc;
    }
    rc = ensure_lumped(d, who);
    if (rc) return rc;
    const FrictionOff no_friction(c);   // (the frictionless figure)
    const int n = d->n, S = c->S(), g = blocks_of(n);
    DevBuf<double> x, y;
    HIP_TRY(c, x.alloc((size_t)n));
    HIP_TRY(c, y.alloc((size_t)n));
    auto normalise = [&]() -> int {   // x <- x / sqrt(x . m x), zero on the Dirichlet dofs
        double mm = 0.0;
        hipLaunchKernelGGL(k_dynamics_mdot, dim3(g), dim3(256), 0, c->stream, n, x.p, d->m.p, d->kep.p);
        HIP_TRY(c, hipGetLastError());
        const int r = sum_blocks(c, d->kep.p, g, &mm);
        if (r) return r;
        hipLaunchKernelGGL(k_dynamics_scale, dim3(g), dim3(256), 0, c->stream, n, S, 1.0 / std::sqrt(mm), dmask_of(c), x.p);
        HIP_TRY(c, hipGetLastError());
        return (int)FH_OK;
    };
    hipLaunchKernelGGL(k_dynamics_fill, dim3(g), dim3(256), 0, c->stream, n, x.p);
    hipLaunchKernelGGL(k_dynamics_scale, dim3(g), dim3(256), 0, c->stream, n, S, 1.0, dmask_of(c), x.p);
    HIP_TRY(c, hipGetLastError());
    rc = normalise();
    if (rc) return rc;
    double rq = 0.0;
    for (uint32_t it = 0; it < iterations; ++it) {
        rc = fh_apply_tangent_dev(c, x.p, y.p);
        if (rc) return rc;
        rc = dot(d, x.p, y.p, &rq);   // x is m-normalised: the Rayleigh quotient of (T, m)
        if (rc) return rc;
        hipLaunchKernelGGL(k_dynamics_divide, dim3(g), dim3(256), 0, c->stream, n, S, dmask_of(c), y.p, d->m.p, x.p);
        HIP_TRY(c, hipGetLastError());
        rc = normalise();
        if (rc) return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!(rq > 0.0) || !std::isfinite(rq)) return c->fail(FH_DYNAMICS_NONFINITE, std::string(who) + ": the Rayleigh quotient is not positive and finite");
    *omega_max = std::sqrt(rq);
    if (!first_order(d)) *dt_crit = d->eta_k != 0.0 ? damped_dt_crit(*omega_max, d->eta_k) : 2.0 / *omega_max;
    else *dt_crit = d->fo_scheme == FH_FO_RKL ? ((double)d->stages * (double)d->stages + (double)d->stages) / (*omega_max * *omega_max) : HUGE_VAL;
    return FH_OK;
}

}  // extern "C"
