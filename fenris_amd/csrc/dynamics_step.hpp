// Time integration (engine_dynamics.hip): the arithmetic of one central-difference launch per dof -- the acceleration, the kick and the
// drift -- as the fused node pass over the tile partials (k_dynamics_from_partials, vector_tiles.hip) and the stand-alone kernel
// (k_dynamics_update, dynamics_kernels.hpp) share it; and the same for one stage of a first-order Runge-Kutta-Legendre step (fo_dof:
// k_first_order_from_partials, k_first_order_update).
#pragma once
#include <hip/hip_runtime.h>

namespace fenris_hip {

// what one launch of the central-difference update does per dof (velocity-Verlet: a kick of dt/2, a drift of dt, a kick of dt/2)
enum {
    DYN_ACCEL = 1,     // a = (lf f - r) / m from the residual at the context's u (Dirichlet dofs: 0)
    DYN_COMPLETE = 2,  // v = v_h + dt/2 a: the second kick (without it DYN_ACCEL forms a_0 and leaves v)
    DYN_STORE = 4,     // v and a are stored and the workgroup leaves its partial of sum m v^2 (the end of a call, or a record)
    DYN_ADVANCE = 8    // the next step's first kick and drift: v_h = v + dt/2 a, u += dt v_h; v_h is stored in v
};

// the load lf_step f of a launch, as every kernel of the integrators takes it
struct StepLoad {
    const double* f;            // load, S N (null: zero)
    const double* lf;           // load factors on the device (null: 1) ...
    unsigned long long lf_count, step;   // ... lf[min(step, lf_count - 1)]
};
__device__ __forceinline__ double load_factor_at(const StepLoad& l, unsigned long long step) {
    return l.lf ? l.lf[step < l.lf_count ? step : l.lf_count - 1] : 1.0;
}

struct DynStep {
    double dt, half_dt;
    StepLoad load;              // load.step: the global index of the step whose acceleration is formed
    const double* m;            // row-sum lumped mass, S N
    const unsigned char* dmask; // N Dirichlet bytes, the held components of each node (dof_fixed, device_common.hpp; null: none)
    double *u, *v, *a;          // S N each: the context's u; v holds v_h between the launches of a call
    double* ke_partial;         // DYN_STORE: one partial per workgroup
    int flags;
    double eta_m = 0.0;         // Rayleigh mass damping (fh_dynamics_set_damping); 0: the arithmetic of the undamped step, bit for bit
    // prescribed motion of the Dirichlet dofs (fh_dynamics_set_boundary_motion; bm_dir null: they are held): direction and the u_0 of
    // fh_dynamics_set_state, S N each, and for the DYN_ADVANCE of this launch, from step k to k + 1, g_{k+1} - g_0 and (g_{k+1} - g_k) / dt,
    // both formed on the host
    const double* bm_dir = nullptr;
    const double* bm_u0 = nullptr;
    double bm_g = 0.0, bm_rate = 0.0;
};

template <class P>   // (DynStep, or FoStage below)
__device__ __forceinline__ double dyn_load_factor(const P& p) { return load_factor_at(p.load, p.load.step); }
// the three pieces every route shares: the same bits however a run is cut into calls and records
__device__ __forceinline__ double dyn_accel(double lf, double f, double r, double m) { return fma(lf, f, -r) / m; }
__device__ __forceinline__ double dyn_kick(double v, double a, double half_dt) { return fma(half_dt, a, v); }
__device__ __forceinline__ double dyn_drift(double u, double vh, double dt) { return fma(dt, vh, u); }
// ... and with Rayleigh damping C = eta_m M + eta_k T(u) on the lumped mass: r holds r(u) + eta_k T(u) w already (w = v_h, the velocity the
// handle keeps between launches; w = v_0 for a_0), so the stiffness part stays explicit; the mass part is implicit in v_{n+1} = v_h + dt/2 a:
// a = ((lf f - r) / m - eta_m v_h) / (1 + eta_m dt/2).  complete = false: a_0 = (lf f - r) / m - eta_m v_0, exact, no divisor.
__device__ __forceinline__ double dyn_accel_damped(double lf, double f, double r, double m, double v, double eta_m, double half_dt, bool complete) {
    const double a = fma(-eta_m, v, fma(lf, f, -r) / m);
    return complete ? a / fma(eta_m, half_dt, 1.0) : a;
}

// one dof of a launch: r is read only with DYN_ACCEL; returns the dof's m v^2 (DYN_STORE, else 0)
__device__ __forceinline__ double dyn_dof(const DynStep& p, size_t i, bool fixed, double lf, double r) {
    if (fixed && p.bm_dir) {   // moved along its prescribed path: u a pure function of the step, v the half-step velocity of the boundary
        if (p.flags & DYN_ADVANCE) {
            const double dir = p.bm_dir[i];
            p.u[i] = fma(p.bm_g, dir, p.bm_u0[i]);
            p.v[i] = p.bm_rate * dir;
        }
        if (p.flags & (DYN_STORE | DYN_ACCEL)) p.a[i] = 0.0;   // (DYN_STORE keeps v; the kinetic energy counts the free dofs only)
        return 0.0;
    }
    if (fixed) {   // held at the u of fh_dynamics_set_state: u is not touched
        if (p.flags & (DYN_STORE | DYN_ADVANCE)) p.v[i] = 0.0;
        if (p.flags & (DYN_STORE | DYN_ACCEL)) p.a[i] = 0.0;
        return 0.0;
    }
    double v = p.v[i], a;
    if (p.flags & DYN_ACCEL) {
        a = p.eta_m != 0.0 ? dyn_accel_damped(lf, p.load.f ? p.load.f[i] : 0.0, r, p.m[i], v, p.eta_m, p.half_dt, (p.flags & DYN_COMPLETE) != 0)
                           : dyn_accel(lf, p.load.f ? p.load.f[i] : 0.0, r, p.m[i]);
        if (p.flags & DYN_COMPLETE) v = dyn_kick(v, a, p.half_dt);
    } else {
        a = p.a[i];
    }
    double ke = 0.0;
    if (p.flags & DYN_STORE) {
        p.v[i] = v;
        p.a[i] = a;
        ke = p.m[i] * (v * v);
    } else if ((p.flags & DYN_ACCEL) && !(p.flags & DYN_COMPLETE)) {
        p.a[i] = a;
    }
    if (p.flags & DYN_ADVANCE) {
        const double vh = dyn_kick(v, a, p.half_dt);
        p.v[i] = vh;
        p.u[i] = dyn_drift(p.u[i], vh, p.dt);
    }
    return ke;
}

// ---- first order: M du/dt + r(u) = lf f.  One launch is one stage of a Runge-Kutta-Legendre step of s stages (s = 1: forward Euler), or
// the rate L(u) = (lf f - r(u)) / m alone
enum {
    FO_FIRST = 1,  // stage 1: Y_1 = fma(mut_dt, L(Y_0), Y_0) -- prev is not read
    FO_KEEP = 2,   // a later stage of the step reads Y_{j-1}: prev takes the u this stage read
    FO_STORE = 4,  // the workgroup leaves its partial of sum m y^2 over all its dofs (the last stage of a recorded step)
    FO_RATE = 8    // no stage: rate takes L(u) (Dirichlet dofs: 0) and u stays
};

struct FoStage {
    double mut_dt, mu, nu;      // mu_j w1 dt, mu_j, nu_j (stage 1: w1 dt; mu and nu are not read)
    StepLoad load;              // load.step: the index of the state the step starts from
    const double* m;            // row-sum lumped mass, S N
    const unsigned char* dmask; // N Dirichlet bytes, the held components of each node (dof_fixed, device_common.hpp; null: none)
    double *u, *prev;           // S N each: the context's u holds Y_{j-1} and takes Y_j; prev holds Y_{j-2}
    double* rate;               // FO_RATE
    double* partial;            // FO_STORE: one partial per workgroup
    int flags;
};

// one dof of a stage: returns the dof's m y^2 (FO_STORE, else 0); a Dirichlet dof keeps its u
__device__ __forceinline__ double fo_dof(const FoStage& p, size_t i, bool fixed, double lf, double r) {
    if (p.flags & FO_RATE) {
        p.rate[i] = fixed ? 0.0 : dyn_accel(lf, p.load.f ? p.load.f[i] : 0.0, r, p.m[i]);
        return 0.0;
    }
    const double m = p.m[i], u = p.u[i];
    double y = u;
    if (!fixed) {
        const double w = dyn_accel(lf, p.load.f ? p.load.f[i] : 0.0, r, m);
        y = (p.flags & FO_FIRST) ? fma(p.mut_dt, w, u) : fma(p.mut_dt, w, fma(p.mu, u, p.nu * p.prev[i]));
        if (p.flags & FO_KEEP) p.prev[i] = u;
        p.u[i] = y;
    }
    return (p.flags & FO_STORE) ? m * (y * y) : 0.0;
}

}  // namespace fenris_hip
