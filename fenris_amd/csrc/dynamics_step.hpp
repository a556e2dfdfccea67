// Time integration (engine_dynamics.hip): the arithmetic of one central-difference launch per dof -- the acceleration, the kick and the
// drift -- as the fused node pass over the tile partials (k_dynamics_from_partials, vector_tiles.hip) and the stand-alone kernel
// (k_dynamics_update, dynamics_kernels.hpp) share it.
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

struct DynStep {
    double dt, half_dt;
    const double* f;            // load, S N (null: zero)
    const double* lf;           // load factors on the device (null: 1) ...
    unsigned long long lf_count, step;   // ... lf[min(step, lf_count - 1)], step the global index of the step whose acceleration is formed
    const double* m;            // row-sum lumped mass, S N
    const unsigned char* dmask; // N membership flags of the Dirichlet nodes (null: none)
    double *u, *v, *a;          // S N each: the context's u; v holds v_h between the launches of a call
    double* ke_partial;         // DYN_STORE: one partial per workgroup
    int flags;
};

__device__ __forceinline__ double dyn_load_factor(const DynStep& p) {
    return p.lf ? p.lf[p.step < p.lf_count ? p.step : p.lf_count - 1] : 1.0;
}
// the three pieces every route shares: the same bits however a run is cut into calls and records
__device__ __forceinline__ double dyn_accel(double lf, double f, double r, double m) { return fma(lf, f, -r) / m; }
__device__ __forceinline__ double dyn_kick(double v, double a, double half_dt) { return fma(half_dt, a, v); }
__device__ __forceinline__ double dyn_drift(double u, double vh, double dt) { return fma(dt, vh, u); }

// one dof of a launch: r is read only with DYN_ACCEL; returns the dof's m v^2 (DYN_STORE, else 0)
__device__ __forceinline__ double dyn_dof(const DynStep& p, size_t i, bool fixed, double lf, double r) {
    if (fixed) {   // held at the u of fh_dynamics_set_state: u is not touched
        if (p.flags & (DYN_STORE | DYN_ADVANCE)) p.v[i] = 0.0;
        if (p.flags & (DYN_STORE | DYN_ACCEL)) p.a[i] = 0.0;
        return 0.0;
    }
    double v = p.v[i], a;
    if (p.flags & DYN_ACCEL) {
        a = dyn_accel(lf, p.f ? p.f[i] : 0.0, r, p.m[i]);
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

}  // namespace fenris_hip
