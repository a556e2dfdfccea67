// Time integration on the device: M a + r(u) = lf f with the context's residual r and the mass of fh_set_mass_density, by central
// differences (velocity-Verlet form, row-sum lumped mass), Newmark(beta, gamma) or backward Euler (one Newton solve per step: newton_run
// of engine_newton.hip on alpha = 1, beta = newmark_beta dt^2); and the first-order problem M du/dt + r(u) = lf f on the same handle, by
// Runge-Kutta-Legendre super-steps (one stage: forward Euler; lumped mass) or the theta method (newton_run on alpha = 1, beta = theta dt);
// the handle, the step loops, the records and the C ABI.
// The frame the four step loops (explicit_steps, implicit_steps, first_order_explicit_steps, first_order_theta_steps) are built from: one
// key of what m and a_n were formed for (DynKey), one launcher of the per-dof kernels (launch_dofs), one description of the load and of
// the boundary motion of a launch (load_of, motion_args), one initial right-hand side and one solve on M (initial_rhs, solve_mass), one
// Newton step with its roll-back (newton_step) and one record tail (record_due, check_record_finite, write_record).
#include "engine_internal.hpp"

#include "dynamics_kernels.hpp"

#include <cmath>

// what m (mass_inputs_equal) and a_n (==; first order: the rate, kept in v) were formed for: struct_gen (operator, table, mask), topo_gen,
// geom_gen, density_gen, dirichlet_gen, the u_gen this handle left behind, and the contact_gen of fh_set_obstacles with the friction_gen
// of fh_set_friction (contact_key), and the expansion_gen of fh_set_element_expansion (the residual of every elastic operator sees the field)
struct DynKey {
    unsigned long long struct_gen = ~0ull, topo_gen = ~0ull, geom_gen = ~0ull, density_gen = ~0ull, dirichlet_gen = ~0ull, u_gen = ~0ull, contact = ~0ull,
                       expansion = ~0ull;
    static DynKey now(const fh_ctx* c) {
        return {c->struct_gen, c->topo_gen, c->geom_gen, c->density_gen, c->dirichlet_gen, c->u_gen, contact_key(c), expansion_key(c, false)};
    }
    bool mass_inputs_equal(const DynKey& o) const {
        return struct_gen == o.struct_gen && topo_gen == o.topo_gen && geom_gen == o.geom_gen && density_gen == o.density_gen &&
               dirichlet_gen == o.dirichlet_gen;
    }
    bool operator==(const DynKey& o) const { return mass_inputs_equal(o) && u_gen == o.u_gen && contact == o.contact && expansion == o.expansion; }
};

// the slots of fh_dynamics_step's stats
enum { STAT_STEPS, STAT_RESIDUALS, STAT_NEWTON, STAT_PCG, STAT_RECORDS, STAT_COUNT };

struct fh_dynamics {
    fh_ctx* c = nullptr;
    fh_dynamics_settings s{};          // (a first-order handle keeps its dt and Newton arguments here; s.scheme is not read then)
    int fo_scheme = -1;                // FH_FO_RKL or FH_FO_THETA; -1: the second-order problem of s.scheme
    double theta = 1.0;
    uint32_t stages = 1;
    bool state_check_pending = true;   // first order: no step call has checked the state since fh_dynamics_set_state
    unsigned long long topo_gen = 0;   // the context's mesh at creation: fh_set_mesh* invalidates the handle
    int n = 0;                         // S N at creation
    DevBuf<double> v, a, m, f, lf, r, rpart, kep, u_ref, u_prev, work, load;
    std::vector<double> h_lf;
    bool has_f = false;
    uint64_t step = 0;                 // steps taken since fh_dynamics_set_state
    DynKey m_key, a_key;               // what m and a_n (first order: the rate) were formed for
    // a_n is to be formed again although a_key holds: set by fh_dynamics_set_load, by fh_dynamics_set_damping and
    // fh_dynamics_set_slip_velocity when a value changes, and by fh_dynamics_set_boundary_motion (set, or a set one cleared)
    bool a_stale = true;
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

// one launch of a per-dof kernel: a thread per dof of the handle, on the context's stream; the launch's own status, nothing is waited for
template <class K, class... Args>
int launch_dofs(fh_dynamics* d, K kernel, Args... args) {
    fh_ctx* c = d->c;
    hipLaunchKernelGGL(kernel, dim3(blocks_of(d->n)), dim3(256), 0, c->stream, args...);
    HIP_TRY(c, hipGetLastError());
    return FH_OK;
}

// the load lf_step f as the kernels take it
StepLoad load_of(const fh_dynamics* d, uint64_t step) { return {d->has_f ? d->f.p : nullptr, d->h_lf.empty() ? nullptr : d->lf.p, d->h_lf.size(), step}; }

bool boundary_motion(const fh_dynamics* d) { return !d->bm_factor.empty(); }
// g_n - g_0, formed on the host: a pure function of n
double motion_factor(const fh_dynamics* d, uint64_t n) { return d->bm_factor[(size_t)std::min<uint64_t>(n, d->bm_factor.size() - 1)]; }
double motion_offset(const fh_dynamics* d, uint64_t n) { return motion_factor(d, n) - d->bm_factor[0]; }
// the prescribed motion of the Dirichlet dofs as a launch takes it (dir null: they are held); `advance`: the launch moves them from `step`
// to step + 1 and takes g_{step+1} - g_0 and (g_{step+1} - g_step) / dt, else both stay zero
struct MotionArgs { const double *dir = nullptr, *u0 = nullptr; double g = 0.0, rate = 0.0; };
MotionArgs motion_args(const fh_dynamics* d, uint64_t step, bool advance) {
    MotionArgs m;
    if (!boundary_motion(d)) return m;
    m.dir = d->bm_dir.p;
    m.u0 = d->bm_u0.p;
    if (advance) {
        m.g = motion_offset(d, step + 1);
        m.rate = (motion_factor(d, step + 1) - motion_factor(d, step)) / d->s.dt;
    }
    return m;
}

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

// y += s T(u) x on the free dofs, T(u) x through tmp: the stiffness part of the damping term on the routes off the tiles and in the implicit
// schemes (tangent_summed, engine_vector.hip: no contact term); waits for the device
int add_tangent(fh_dynamics* d, double s, const double* x, double* tmp, double* y) {
    fh_ctx* c = d->c;
    const int rc = tangent_summed(c, x, tmp);
    return rc ? rc : launch_dofs(d, k_dynamics_axpy, d->n, c->S(), s, dmask_of(c), tmp, y);
}

// the scope check of the handle's configuration: the prescribed boundary motions no remedy is chosen for, friction and obstacle paths on
// a first-order handle, and what the folding of a frozen C into newton_run's arguments cannot express
int config_in_scope(fh_dynamics* d, const char* who) {
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

// x . y in a fixed order: the workgroups' partials, summed on the host in index order (the host waits)
int dot(fh_dynamics* d, const double* x, const double* y, double* out) {
    const int rc = launch_dofs(d, k_kinetic_partials, d->n, x, y, d->kep.p);
    return rc ? rc : sum_partials(d->c, d->kep.p, blocks_of(d->n), 1, out);
}

// a_n (first order: the rate) belongs to the state as it stands, or does from now on
bool a_current(const fh_dynamics* d) { return DynKey::now(d->c) == d->a_key && !d->a_stale; }
void a_formed(fh_dynamics* d) {
    d->a_key = DynKey::now(d->c);
    d->a_stale = false;
}

// the row-sum lumped mass m = M 1 (no Dirichlet rows take part) for the current mesh, table, mask and density; every free dof must have m > 0
int ensure_lumped(fh_dynamics* d, const char* who) {
    fh_ctx* c = d->c;
    const DynKey k = DynKey::now(c);
    if (k.mass_inputs_equal(d->m_key)) return FH_OK;
    // (with damping or friction a_n is not formed again for what the handle itself moves -- remember_u -- and the walk below moves struct_gen on a
    // rule-set table: an a_n that is current on entry stays current)
    const bool keep_a = velocity_term(d) && a_current(d);
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
        if (!dof_fixed_at(hm.data(), i, S) && !(h[(size_t)i] > 0.0))
            return c->fail(FH_UNSUPPORTED, std::string(who) + ": the row-sum lumped mass of dof " + std::to_string(i) + " (node " + std::to_string(i / S) +
                                               ") is " + std::to_string(h[(size_t)i]) + ", not positive: the explicit schemes need another lumping on this element kind");
    d->m_key = k;
    if (keep_a) a_formed(d);
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
    p.load = load_of(d, step);
    p.m = d->m.p;
    p.dmask = dmask_of(c);
    p.u = c->u.p;
    p.v = d->v.p;
    p.a = d->a.p;
    p.ke_partial = d->kep.p;
    p.flags = flags;
    p.eta_m = d->eta_m;
    // the drift of this launch: from `step` to step + 1 (without DYN_ADVANCE the fixed branch only leaves v alone)
    const MotionArgs mo = motion_args(d, step, (flags & DYN_ADVANCE) != 0);
    p.bm_dir = mo.dir;
    p.bm_u0 = mo.u0;
    p.bm_g = mo.g;
    p.bm_rate = mo.rate;
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
        ++stats[STAT_RESIDUALS];
        if (tiles) {
            HIP_TRY(c, vector_tiles_dynamics_node_pass(c->stream, S, (int)c->N, c->vt.v, d->rpart.p, p, contact_table(c)));
            c->last_kernel = d->eta_k != 0.0 ? "k_damped_pass_tiled + k_dynamics_from_partials" : "k_element_pass_tiled + k_dynamics_from_partials";
            if (ke_count) *ke_count = vector_tiles_operator_partials((int)c->N);
            if (flags & DYN_ADVANCE) ++c->u_gen;
            return FH_OK;
        }
        rc = residual_summed(c, d->r.p);
        if (rc) return rc;
        if (d->eta_k != 0.0) {   // r += eta_k T(u) v
            rc = add_tangent(d, d->eta_k, d->v.p, d->work.p, d->r.p);
            if (rc) return rc;
        }
        c->last_kernel = contact_table(c).count ? "k_residual_elements + k_vector_from_elements_soa + k_contact_force + k_dynamics_update"
                                                : "k_residual_elements + k_vector_from_elements_soa + k_dynamics_update";
    }
    const int rl = launch_dofs(d, k_dynamics_update, n, S, d->r.p, p);
    if (rl) return rl;
    if (ke_count) *ke_count = blocks_of(n);
    if (flags & DYN_ADVANCE) ++c->u_gen;
    return FH_OK;
}

double load_factor(const fh_dynamics* d, uint64_t step) { return d->h_lf.empty() ? 1.0 : d->h_lf[(size_t)std::min<uint64_t>(step, d->h_lf.size() - 1)]; }

// the rest of a row whose [0] holds the summed quadratic form (halved here): stored energy (with obstacles set: plus the contact energy
// E_c) and load potential of the state after `step` steps, into row[1..3]
int record_rest(fh_dynamics* d, uint64_t step, double* row) {
    fh_ctx* c = d->c;
    row[0] *= 0.5;
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

// x . M x with the consistent mass, M x through d->work (the host waits)
int consistent_form(fh_dynamics* d, const double* x, double* out) {
    const int rc = mass_full(d->c, x, nullptr, d->work.p);
    return rc ? rc : dot(d, x, d->work.p, out);
}

// ---- the record tail of the four loops: a record is due after every record_every-th step of a call and after its last.  Each loop
// keeps its own order of the check and the write, which a caller sees in records, stats and *steps_done (include/fenris_hip.h says what
// *steps_done is after FH_DYNAMICS_NONFINITE): Newmark and backward Euler write the row and then check it, the step already committed;
// central differences, RKL and theta check and then write, and the first two commit the step only behind a clean record.
const char* SECOND_ORDER_ENERGIES = "the kinetic or stored energy";
const char* FIRST_ORDER_ENERGIES = "1/2 u^T B u or the stored energy";
bool record_due(uint64_t j, uint64_t num_steps, uint64_t record_every) { return j + 1 == num_steps || (record_every && (j + 1) % record_every == 0); }
int check_record_finite(fh_dynamics* d, uint64_t step, const double* row, const char* what) {
    if (std::isfinite(row[0]) && std::isfinite(row[1])) return FH_OK;
    return d->c->fail(FH_DYNAMICS_NONFINITE, std::string(WHO) + ": " + what + " after step " + std::to_string(step) + " is not finite");
}
void write_record(const double* row, double* records, uint64_t* stats) {
    if (records) std::copy(row, row + 4, records + 4 * stats[STAT_RECORDS]);
    ++stats[STAT_RECORDS];
}

// ---- the right-hand side of the state as it stands, shared by a_0 of Newmark and the rate of theta
// b = lf_n f - r(u_n) on the free dofs into d->work (the residual summed into d->r and counted)
int initial_rhs(fh_dynamics* d, uint64_t* stats) {
    fh_ctx* c = d->c;
    const int rc = residual_summed(c, d->r.p);
    if (rc) return rc;
    ++stats[STAT_RESIDUALS];
    return launch_dofs(d, k_dynamics_rhs, d->n, c->S(), load_of(d, d->step), dmask_of(c), d->r.p, d->work.p);
}
// ... refused when it is not finite (an inverted NeoHookean state makes r NaN: reported as such, not as a breakdown of the PCG or of Newton)
int refuse_nonfinite_rhs(fh_dynamics* d, const double* b) {
    double b2 = 0.0;
    const int rc = dot(d, b, b, &b2);
    if (rc || std::isfinite(b2)) return rc;
    return d->c->fail(FH_DYNAMICS_NONFINITE, std::string(WHO) + ": the residual of the initial state is not finite");
}
// ... and M x = d->work on the free dofs from the x given, by the handle's PCG settings (M alone needs no hierarchy: multigrid is Jacobi here)
int solve_mass(fh_dynamics* d, double* x, uint64_t* stats) {
    uint64_t it = 0;
    const int pre = d->s.preconditioner == FH_PRECOND_MULTIGRID ? (int)FH_PRECOND_JACOBI : d->s.preconditioner;
    const int rc = cg_solve_free_dev(d->c, WHO, MF_TANGENT, d->work.p, x, pre, d->s.linear_rel_tol, d->s.linear_max_iter, &it, 1.0, 0.0);
    stats[STAT_PCG] += it;
    return rc;
}

// a_n for the state as it stands, when anything it depends on has changed since it was formed
int ensure_acceleration(fh_dynamics* d, uint64_t* stats) {
    fh_ctx* c = d->c;
    if (a_current(d)) return FH_OK;
    const int n = d->n, S = c->S();
    int rc;
    // (v and a of a Dirichlet dof are zero whatever fh_dynamics_set_state was given; with a boundary motion set v there is the handle's own)
    if (!boundary_motion(d)) {
        rc = launch_dofs(d, k_dynamics_scale, n, S, 1.0, dmask_of(c), d->v.p);
        if (rc) return rc;
    }
    if (explicit_scheme(d)) {
        rc = reset_status(c);
        if (!rc) rc = explicit_launch(d, DYN_ACCEL, d->step, stats, nullptr);
        if (rc) return rc;
    } else {   // Newmark: M a_0 = lf_0 f - r(u_0) on the free dofs; backward Euler keeps no a_0 but refuses the same states
        clock_to_step(d, d->step, false);
        if (friction_active(c)) {   // (the lag state of a_0 is u_0 itself: no slip, no friction force)
            rc = friction_lag_to_u(c, slip_eps(d));
            if (rc) return rc;
        }
        rc = initial_rhs(d, stats);
        if (rc) return rc;
        if (d->eta_k != 0.0 && d->s.scheme == FH_DYN_NEWMARK) {   // M a_0 = lf_0 f - r(u_0) - C v_0: the stiffness part joins the right-hand side
            rc = add_tangent(d, -d->eta_k, d->v.p, d->r.p, d->work.p);
            if (rc) return rc;
        }
        rc = refuse_nonfinite_rhs(d, d->work.p);
        if (rc) return rc;
        HIP_TRY(c, hipMemsetAsync(d->a.p, 0, sizeof(double) * (size_t)n, c->stream));
        if (d->s.scheme == FH_DYN_NEWMARK) {
            rc = solve_mass(d, d->a.p, stats);
            if (rc) return rc;
            if (d->eta_m != 0.0) {   // ... and the mass part leaves the solve: a_0 -= eta_m v_0
                rc = launch_dofs(d, k_dynamics_axpy, n, S, -d->eta_m, dmask_of(c), d->v.p, d->a.p);
                if (rc) return rc;
            }
        }
    }
    a_formed(d);
    return FH_OK;
}

// a_n belongs to the state the handle has just left behind.  With damping or friction (velocity_term) a step's a_{n+1} (formed on v_h)
// is not what ensure_acceleration would form again for the same state (on v_{n+1}), so nothing the steps themselves moved may make it stale: the walk over the groups of a
// rule-set table stages every group and moves struct_gen, which without damping only forms the same a_n once more.
void remember_u(fh_dynamics* d) {
    if (velocity_term(d)) d->a_key = DynKey::now(d->c);   // (with friction the implicit steps move the lag state, and friction_gen, themselves)
    else d->a_key.u_gen = d->c->u_gen;
}

int explicit_steps(fh_dynamics* d, uint64_t num_steps, uint64_t record_every, double* records, uint64_t* done, uint64_t* stats) {
    fh_ctx* c = d->c;
    const uint64_t s0 = d->step;
    int rc = reset_status(c);
    if (rc) return rc;
    rc = explicit_launch(d, DYN_ADVANCE, s0, stats, nullptr);   // the first kick and drift of the call
    if (rc) return rc;
    for (uint64_t j = 0; j < num_steps; ++j) {
        const bool rec = record_due(j, num_steps, record_every);
        int ke_count = 0;
        // (a record needs u_{n+1} for the stored energy and the load potential, so the launch of a record stores and stops; every other
        // launch goes straight on to the next kick and drift)
        rc = explicit_launch(d, DYN_ACCEL | DYN_COMPLETE | (rec ? DYN_STORE : DYN_ADVANCE), s0 + j + 1, stats, rec ? &ke_count : nullptr);
        if (rc) return rc;
        if (!rec) continue;
        double row[4] = {0.0, 0.0, 0.0, 0.0};
        rc = sum_partials(c, d->kep.p, ke_count, 1, &row[0]);   // the host waits here: once per record
        if (!rc) rc = read_status(c, nullptr);
        if (!rc) rc = record_rest(d, s0 + j + 1, row);
        if (!rc) rc = check_record_finite(d, s0 + j + 1, row, SECOND_ORDER_ENERGIES);
        if (rc) return rc;
        write_record(row, records, stats);
        *done = j + 1;
        d->step = s0 + j + 1;
        remember_u(d);
        if (j + 1 < num_steps) {
            rc = reset_status(c);
            if (rc) return rc;
            rc = explicit_launch(d, DYN_ADVANCE, d->step, stats, nullptr);
            if (rc) return rc;
        }
    }
    return FH_OK;
}

// one Newton solve of an implicit step, its counters folded into stats.  A solve that fails leaves the state of the last completed step:
// u comes back from d->u_prev (the host waits), u_gen moves, and the solver's message stands
int newton_step(fh_dynamics* d, double alpha, double beta, const double* load, const double* u_ref, uint64_t* stats) {
    fh_ctx* c = d->c;
    const int n = d->n;
    uint64_t st[4] = {0, 0, 0, 0};   // newton_run's own: [0] iterations, [1] residual evaluations, [2] PCG iterations
    double nm[3] = {0.0, 0.0, 0.0};
    const int rc = newton_run(c, alpha, beta, load, u_ref, d->s.newton_tolerance, d->s.newton_max_iterations, d->s.line_search, d->s.preconditioner,
                              d->s.linear_rel_tol, d->s.linear_max_iter, st, nm);
    stats[STAT_RESIDUALS] += st[1];
    stats[STAT_NEWTON] += st[0];
    stats[STAT_PCG] += st[2];
    if (!rc) return FH_OK;
    const std::string msg = c->err;
    HIP_TRY(c, hipMemcpyAsync(c->u.p, d->u_prev.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    ++c->u_gen;
    return c->fail(rc, msg);
}

// a step that does not complete, for whatever reason, leaves the contact clock of the state that stands: the one place it is put back
struct ClockBack {
    fh_ctx* c;
    double t, t_lag;
    bool armed;
    void restore() { if (armed) contact_set_time(c, t, t_lag); armed = false; }
    ~ClockBack() { restore(); }
};

int implicit_steps(fh_dynamics* d, uint64_t num_steps, uint64_t record_every, double* records, uint64_t* done, uint64_t* stats) {
    fh_ctx* c = d->c;
    const int n = d->n, S = c->S();
    const bool euler = d->s.scheme == FH_DYN_BACKWARD_EULER;
    const double dt = d->s.dt, nb = euler ? 1.0 : d->s.newmark_beta, bdt2 = nb * dt * dt;
    for (uint64_t j = 0; j < num_steps; ++j) {
        const uint64_t g_step = d->step + 1;
        ClockBack clock_back{c, c->contact_t, c->contact_t_lag, true};
        clock_to_step(d, g_step, true);
        int rc;
        if (friction_active(c)) {   // the lag state of the step is u_n: a device copy enqueued with the step
            rc = friction_lag_to_u(c, slip_eps(d));
            if (rc) return rc;
        }
        const MotionArgs mo = motion_args(d, d->step, true);   // (backward Euler alone: the Dirichlet dofs take the prescribed u_{n+1})
        rc = launch_dofs(d, k_newmark_predict, n, S, dt, euler ? 0.0 : dt * dt * (0.5 - nb), dmask_of(c), c->u.p, d->v.p, d->a.p, d->u_ref.p,
                         d->u_prev.p, mo.dir, mo.u0, mo.g);
        if (rc) return rc;
        ++c->u_gen;
        const double* load = nullptr;
        if (d->has_f) {   // the load of the step: lf_{n+1} f
            HIP_TRY(c, hipMemcpyAsync(d->load.p, d->f.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
            rc = launch_dofs(d, k_dynamics_scale, n, S, load_factor(d, g_step), (const unsigned char*)nullptr, d->load.p);
            if (rc) return rc;
            load = d->load.p;
        }
        // Rayleigh damping, C frozen at the start of the step, folded into the four arguments (k_damping_fold; the corrector below takes
        // the unmodified u_ref)
        double alpha = 1.0, beta2 = bdt2;
        const double* u_ref = d->u_ref.p;
        if (d->eta_m != 0.0 || d->eta_k != 0.0) {
            const double gdt = (euler ? 1.0 : d->s.newmark_gamma) * dt;
            alpha = 1.0 + d->eta_m * gdt;
            beta2 = bdt2 + d->eta_k * gdt;
            rc = launch_dofs(d, k_damping_fold, n, S, euler ? 0.0 : dt - gdt, d->eta_m * bdt2 / alpha, bdt2, gdt, dmask_of(c), d->u_ref.p, d->v.p, d->a.p,
                             d->u_ref2.p, d->work.p);
            if (rc) return rc;
            u_ref = d->u_ref2.p;
            if (d->eta_k != 0.0) {   // one application of the linear operator, on w
                rc = tangent_summed(c, d->work.p, d->r.p);
                if (rc) return rc;
                rc = launch_dofs(d, k_damping_load, n, bdt2 * load_factor(d, g_step), load_of(d, g_step).f, d->eta_k, d->r.p, beta2, d->load.p);
                if (rc) return rc;
                load = d->load.p;
            }
        }
        rc = newton_step(d, alpha, beta2, load, u_ref, stats);
        if (rc) {
            clock_back.restore();   // (before the key is taken: an obstacle put back on its path moves contact_gen)
            remember_u(d);
            return rc;
        }
        rc = launch_dofs(d, k_newmark_correct, n, S, euler ? 1 : 0, dt, 1.0 / bdt2, d->s.newmark_gamma, dmask_of(c), c->u.p, d->u_ref.p, d->u_prev.p,
                         d->v.p, d->a.p, boundary_motion(d) ? 1 : 0);
        if (rc) return rc;
        d->step = g_step;
        clock_back.armed = false;
        remember_u(d);
        *done = j + 1;
        if (!record_due(j, num_steps, record_every)) continue;
        double row[4] = {0.0, 0.0, 0.0, 0.0};
        rc = consistent_form(d, d->v.p, &row[0]);   // the consistent kinetic energy 1/2 v . M v
        if (!rc) rc = record_rest(d, g_step, row);
        if (rc) return rc;
        write_record(row, records, stats);
        rc = check_record_finite(d, g_step, row, SECOND_ORDER_ENERGIES);
        if (rc) return rc;
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
    p.load = load_of(d, step);
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
    ++stats[STAT_RESIDUALS];
    if (tiles) {
        HIP_TRY(c, vector_tiles_first_order_node_pass(c->stream, S, (int)c->N, c->vt.v, d->rpart.p, p, contact_table(c)));
        c->last_kernel = "k_element_pass_tiled + k_first_order_from_partials";
        if (count) *count = vector_tiles_operator_partials((int)c->N);
    } else {
        rc = residual_summed(c, d->r.p);
        if (rc) return rc;
        rc = launch_dofs(d, k_first_order_update, n, S, d->r.p, p);
        if (rc) return rc;
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
    if (a_current(d)) return FH_OK;
    const int n = d->n;
    int rc;
    if (d->fo_scheme == FH_FO_RKL) {
        rc = reset_status(c);
        if (!rc) rc = first_order_launch(d, stage_args(d, FO_RATE, d->step, 0.0, 0.0, 0.0), stats, nullptr);
        if (!rc) rc = refuse_nonfinite_rhs(d, d->v.p);
        if (!rc) rc = read_status(c, nullptr);
    } else {
        rc = initial_rhs(d, stats);
        if (!rc) rc = refuse_nonfinite_rhs(d, d->work.p);
        if (rc || !solve) return rc;   // (a step needs the check alone)
        HIP_TRY(c, hipMemsetAsync(d->v.p, 0, sizeof(double) * (size_t)n, c->stream));
        rc = solve_mass(d, d->v.p, stats);
    }
    if (rc) return rc;
    a_formed(d);
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
        const bool rec = record_due(j, num_steps, record_every);
        int count = 0;
        for (uint32_t k = 1; k <= s; ++k) {
            const double mu = (2.0 * k - 1.0) / k, nu = (1.0 - k) / k;
            const int flags = (k == 1 ? FO_FIRST : 0) | (k < s ? FO_KEEP : 0) | (k == s && rec ? FO_STORE : 0);
            rc = first_order_launch(d, stage_args(d, flags, s0 + j, k == 1 ? w1dt : mu * w1dt, mu, nu), stats, &count);
            if (rc) return rc;
        }
        if (!rec) continue;
        double row[4] = {0.0, 0.0, 0.0, 0.0};
        rc = sum_partials(c, d->kep.p, count, 1, &row[0]);   // u^T m u: the host waits here, once per record
        if (!rc) rc = read_status(c, nullptr);
        if (!rc) rc = record_rest(d, s0 + j + 1, row);
        if (!rc) rc = check_record_finite(d, s0 + j + 1, row, FIRST_ORDER_ENERGIES);
        if (rc) return rc;
        write_record(row, records, stats);
        *done = j + 1;   // (the step counter moves only behind a clean record)
        d->step = s0 + j + 1;
        if (j + 1 < num_steps) {
            rc = reset_status(c);
            if (rc) return rc;
        }
    }
    return FH_OK;
}

// theta method: one newton_step per step on alpha = 1, beta = theta dt, u_ref = u_n, from the guess u_n
int first_order_theta_steps(fh_dynamics* d, uint64_t num_steps, uint64_t record_every, double* records, uint64_t* done, uint64_t* stats) {
    fh_ctx* c = d->c;
    const int n = d->n;
    const double dt = d->s.dt, cw = (1.0 - d->theta) / d->theta;
    for (uint64_t j = 0; j < num_steps; ++j) {
        const uint64_t g_step = d->step + 1;
        HIP_TRY(c, hipMemcpyAsync(d->u_prev.p, c->u.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
        int rc;
        if (cw != 0.0) {
            rc = residual_summed(c, d->r.p);
            if (rc) return rc;
            ++stats[STAT_RESIDUALS];
        }
        const double* load = nullptr;
        if (d->has_f || cw != 0.0) {
            rc = launch_dofs(d, k_theta_load, n, load_of(d, d->step), cw, d->r.p, d->load.p);
            if (rc) return rc;
            load = d->load.p;
        }
        rc = newton_step(d, 1.0, d->theta * dt, load, d->u_prev.p, stats);
        if (rc) return rc;
        d->step = g_step;
        *done = j + 1;
        if (!record_due(j, num_steps, record_every)) continue;
        double row[4] = {0.0, 0.0, 0.0, 0.0};
        rc = consistent_form(d, c->u.p, &row[0]);   // u^T M u
        if (!rc) rc = record_rest(d, g_step, row);
        if (!rc) rc = check_record_finite(d, g_step, row, FIRST_ORDER_ENERGIES);
        if (rc) return rc;
        write_record(row, records, stats);
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
    d->a_key.u_gen = ~0ull;
    d->state_check_pending = true;
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
    d->a_stale = true;
    return FH_OK;
}

int set_motion_common(fh_dynamics* d, const double* direction, const double* factor, uint64_t count, hipMemcpyKind kind) {
    fh_ctx* c = d->c;
    const char* who = "fh_dynamics_set_boundary_motion";
    if (!direction) {
        if (boundary_motion(d)) d->a_stale = true;   // a_n is formed again, as after fh_dynamics_set_load
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
    d->a_stale = true;
    return FH_OK;
}

int state_common(fh_dynamics* d, double* u, double* v, double* a, double* time, uint64_t* step, hipMemcpyKind kind) {
    fh_ctx* c = d->c;
    int rc = dyn_ready(d, "fh_dynamics_state");
    if (rc) return rc;
    const size_t bytes = sizeof(double) * (size_t)d->n;
    if (boundary_motion(d) || (first_order(d) && contact_has_paths(c))) {   // (out of scope whatever is asked for)
        rc = config_in_scope(d, "fh_dynamics_state");
        if (rc) return rc;
    }
    if ((first_order(d) ? v : a) && c->has_u && c->N) {   // a_n of the state as it stands (a_0 before the first step); first order: the rate
        uint64_t st[STAT_COUNT] = {};
        rc = config_in_scope(d, "fh_dynamics_state");
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
    if (eta_mass != d->eta_m || eta_stiffness != d->eta_k) d->a_stale = true;   // a_n is formed again, as after fh_dynamics_set_load
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
    if (eps_v != d->eps_v) d->a_stale = true;   // a_n is formed again, as after fh_dynamics_set_load
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
    uint64_t st[STAT_COUNT] = {}, done = 0;
    if (steps_done) *steps_done = 0;
    if (stats) std::fill(stats, stats + STAT_COUNT, 0);
    int rc = dyn_ready(d, WHO);
    if (rc) return rc;
    if (c->N == 0 || num_steps == 0) return FH_OK;
    if (!c->has_u) {
        rc = set_state_common(d, nullptr, nullptr, hipMemcpyHostToDevice);
        if (rc) return rc;
    }
    rc = config_in_scope(d, WHO);
    if (rc) return rc;
    if (explicit_scheme(d)) rc = ensure_lumped(d, WHO);
    if (first_order(d)) {   // (the steps do not read the rate: the state is checked once)
        if (!rc && d->state_check_pending) rc = ensure_rate(d, false, st);
        if (!rc) {
            d->state_check_pending = false;
            rc = explicit_scheme(d) ? first_order_explicit_steps(d, num_steps, record_every, records, &done, st)
                                    : first_order_theta_steps(d, num_steps, record_every, records, &done, st);
        }
    } else {
        if (!rc) rc = ensure_acceleration(d, st);
        if (!rc)
            rc = explicit_scheme(d) ? explicit_steps(d, num_steps, record_every, records, &done, st)
                                    : implicit_steps(d, num_steps, record_every, records, &done, st);
    }
    st[STAT_STEPS] = done;
    if (steps_done) *steps_done = done;
    if (stats) std::copy(st, st + STAT_COUNT, stats);
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
    const int n = d->n, S = c->S();
    DevBuf<double> x, y;
    HIP_TRY(c, x.alloc((size_t)n));
    HIP_TRY(c, y.alloc((size_t)n));
    auto normalise = [&]() -> int {   // x <- x / sqrt(x . m x), zero on the Dirichlet dofs
        double mm = 0.0;
        int r = launch_dofs(d, k_dynamics_mdot, n, x.p, d->m.p, d->kep.p);
        if (!r) r = sum_partials(c, d->kep.p, blocks_of(n), 1, &mm);
        return r ? r : launch_dofs(d, k_dynamics_scale, n, S, 1.0 / std::sqrt(mm), dmask_of(c), x.p);
    };
    rc = launch_dofs(d, k_dynamics_fill, n, x.p);
    if (!rc) rc = launch_dofs(d, k_dynamics_scale, n, S, 1.0, dmask_of(c), x.p);
    if (!rc) rc = normalise();
    if (rc) return rc;
    double rq = 0.0;
    for (uint32_t it = 0; it < iterations; ++it) {
        rc = fh_apply_tangent_dev(c, x.p, y.p);
        if (rc) return rc;
        rc = dot(d, x.p, y.p, &rq);   // x is m-normalised: the Rayleigh quotient of (T, m)
        if (rc) return rc;
        rc = launch_dofs(d, k_dynamics_divide, n, S, dmask_of(c), y.p, d->m.p, x.p);
        if (!rc) rc = normalise();
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
