// Time integration (engine_dynamics.hip): the central-difference update on a summed residual (the arithmetic of dynamics_step.hpp, which
// the fused node pass k_dynamics_from_partials of vector_tiles.hip shares), the Newmark predictor and corrector, the kinetic-energy
// partials and the vector kernels of the power iteration.  No atomics: every sum is a fixed tree per workgroup, the partials summed in index order.
#pragma once
#include <hip/hip_runtime.h>

#include "dynamics_step.hpp"
#include "element_pass.hpp"

namespace fenris_hip {

// the central-difference update on a residual that is already summed (r: S N, read with DYN_ACCEL): the routes off the tiles -- Hex27,
// Quad9, the quadratic simplices, rule-set tables, tiles that could not be built -- and the first kick and drift of a call on every route
static __global__ void __launch_bounds__(256) k_dynamics_update(int n, int S, const double* r, const DynStep p) {
    __shared__ double red[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    double ke = 0.0;
    if (i < n) ke = dyn_dof(p, (size_t)i, dof_fixed_at(p.dmask, i, S), dyn_load_factor(p), (p.flags & DYN_ACCEL) ? r[i] : 0.0);
    if (p.flags & DYN_STORE) {
        const double tot = block_sum_256(ke, red);
        if (threadIdx.x == 0) p.ke_partial[blockIdx.x] = tot;
    }
}

// one stage of a Runge-Kutta-Legendre step, or the rate alone (fo_dof, dynamics_step.hpp), on a residual that is already summed: the routes
// off the tiles, as k_dynamics_update serves them
static __global__ void __launch_bounds__(256) k_first_order_update(int n, int S, const double* r, const FoStage p) {
    __shared__ double red[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    double q = 0.0;
    if (i < n) q = fo_dof(p, (size_t)i, dof_fixed_at(p.dmask, i, S), dyn_load_factor(p), r[i]);
    if (p.flags & FO_STORE) {
        const double tot = block_sum_256(q, red);
        if (threadIdx.x == 0) p.partial[blockIdx.x] = tot;
    }
}

// the load of a theta step: g = (lf_{n+1} + c lf_n) f - c r(u_n), c = (1 - theta) / theta (c == 0: r is not read and may be null)
static __global__ void __launch_bounds__(256) k_theta_load(int n, const StepLoad l, double c, const double* r, double* g) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double l0 = load_factor_at(l, l.step), l1 = load_factor_at(l, l.step + 1);
    const double lfv = fma(c, l0, l1) * (l.f ? l.f[i] : 0.0);
    g[i] = c != 0.0 ? fma(-c, r[i], lfv) : lfv;
}

// Newmark predictor: u_ref = u + dt v + dt^2 (1/2 - beta) a (backward Euler: c2 = 0), and the Newton guess: the context's u takes u_ref on
// the free dofs and keeps its Dirichlet entries; u_prev keeps u_n.  bm_dir (may be null; backward Euler only): the Dirichlet dofs follow a
// prescribed motion -- u_ref as on a free dof, and the guess takes the prescribed u_{n+1} = fma(bm_g, dir, u_0), which Newton then holds
static __global__ void __launch_bounds__(256) k_newmark_predict(int n, int S, double dt, double c2, const unsigned char* dmask, double* u,
                                                                const double* v, const double* a, double* u_ref, double* u_prev,
                                                                const double* bm_dir, const double* bm_u0, double bm_g) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double un = u[i];
    u_prev[i] = un;
    const bool fixed = dof_fixed_at(dmask, i, S);
    if (fixed && bm_dir) {
        u_ref[i] = fma(c2, a[i], fma(dt, v[i], un));
        u[i] = fma(bm_g, bm_dir[i], bm_u0[i]);
        return;
    }
    const double ur = fixed ? un : fma(c2, a[i], fma(dt, v[i], un));
    u_ref[i] = ur;
    u[i] = ur;
}

// Newmark corrector on the solved u: a_new = (u - u_ref) inv_bdt2, v += dt ((1 - gamma) a + gamma a_new); backward Euler (euler != 0):
// v = (u - u_prev) / dt, a = (v - v_old) / dt.  Dirichlet dofs: v = a = 0, or with `moved` (a prescribed boundary motion, backward Euler)
// the kinematics of a free dof.
static __global__ void __launch_bounds__(256) k_newmark_correct(int n, int S, int euler, double dt, double inv_bdt2, double gamma,
                                                                const unsigned char* dmask, const double* u, const double* u_ref,
                                                                const double* u_prev, double* v, double* a, int moved) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (!moved && dof_fixed_at(dmask, i, S)) {
        v[i] = 0.0;
        a[i] = 0.0;
        return;
    }
    if (euler) {
        const double vn = (u[i] - u_prev[i]) / dt;
        a[i] = (vn - v[i]) / dt;
        v[i] = vn;
    } else {
        const double an = (u[i] - u_ref[i]) * inv_bdt2, ao = a[i];
        v[i] = fma(dt, fma(gamma, an, (1.0 - gamma) * ao), v[i]);
        a[i] = an;
    }
}

// ---- Rayleigh damping C = eta_m M + eta_k A (fh_dynamics_set_damping)
// y += s x on the free dofs: the damping term joining a summed residual or a right-hand side, and a_0 -= eta_m v_0
static __global__ void __launch_bounds__(256) k_dynamics_axpy(int n, int S, double s, const unsigned char* dmask, const double* x, double* y) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n && !dof_fixed_at(dmask, i, S)) y[i] = fma(s, x[i], y[i]);
}
// the folding of C, frozen at the start of an implicit step, into the Newton arguments.  With v_p = v_n + cv a_n (cv = dt (1 - gamma);
// backward Euler is beta = gamma = 1 on its own predictor: cv = 0) the step's velocity is v_{n+1} = v_p + gamma / (beta dt) (u - u_ref), so
//   u_ref* = u_ref - cref v_p,  cref = eta_m beta dt^2 / (1 + eta_m gamma dt)   (the mass part; Dirichlet dofs keep u_ref: v_p = 0 there)
//   w      = b v_p - gdt u_ref,  b = beta dt^2, gdt = gamma dt                   (the stiffness part's operand: k_damping_load takes A w)
static __global__ void __launch_bounds__(256) k_damping_fold(int n, int S, double cv, double cref, double b, double gdt, const unsigned char* dmask,
                                                             const double* u_ref, const double* v, const double* a, double* u_ref2, double* w) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double vp = dof_fixed_at(dmask, i, S) ? 0.0 : (cv != 0.0 ? fma(cv, a[i], v[i]) : v[i]);
    const double ur = u_ref[i];
    u_ref2[i] = fma(-cref, vp, ur);
    w[i] = fma(b, vp, -gdt * ur);
}
// the folded load f' = (b lf f - eta_k A w) / beta', beta' = b + eta_k gamma dt (blf = b lf_{n+1}; f null: zero)
static __global__ void __launch_bounds__(256) k_damping_load(int n, double blf, const double* f, double eta_k, const double* Aw, double beta2, double* g) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) g[i] = fma(-eta_k, Aw[i], f ? blf * f[i] : 0.0) / beta2;
}

// per-workgroup partials of x . y: the consistent kinetic energy from y = M v, the load potential f . u
static __global__ void __launch_bounds__(256) k_kinetic_partials(int n, const double* x, const double* y, double* partial) {
    __shared__ double red[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const double t = i < n ? x[i] * y[i] : 0.0;
    const double tot = block_sum_256(t, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// b = lf f - r with the rows of the Dirichlet nodes zero: the right-hand side of M a_0 = lf_0 f - r(u_0)
static __global__ void __launch_bounds__(256) k_dynamics_rhs(int n, int S, const StepLoad l, const unsigned char* dmask, const double* r, double* b) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    b[i] = dof_fixed_at(dmask, i, S) ? 0.0 : fma(load_factor_at(l, l.step), l.f ? l.f[i] : 0.0, -r[i]);
}

// x[i] *= s, or x[i] = 0 on the Dirichlet dofs (power iteration on the free dofs; s = 1: v of the Dirichlet dofs cleared; dmask null: the
// scaled load of an implicit step)
static __global__ void __launch_bounds__(256) k_dynamics_scale(int n, int S, double s, const unsigned char* dmask, double* x) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) x[i] = dof_fixed_at(dmask, i, S) ? 0.0 : x[i] * s;
}
// x = y / m on the free dofs, 0 on the Dirichlet dofs (power iteration)
static __global__ void __launch_bounds__(256) k_dynamics_divide(int n, int S, const unsigned char* dmask, const double* y, const double* m, double* x) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) x[i] = dof_fixed_at(dmask, i, S) ? 0.0 : y[i] / m[i];
}
// the start vector of the power iteration: column 0 of fh_eigs_lowest's fill
static __global__ void __launch_bounds__(256) k_dynamics_fill(int n, double* x) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    unsigned long long z = (unsigned long long)i + 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    x[i] = (double)(z >> 11) * 0x1p-52 - 1.0;
}
// one partial per workgroup: x . (m x)
static __global__ void __launch_bounds__(256) k_dynamics_mdot(int n, const double* x, const double* m, double* partial) {
    __shared__ double red[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const double t = i < n ? m[i] * (x[i] * x[i]) : 0.0;
    const double tot = block_sum_256(t, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

}  // namespace fenris_hip
