// Penalty contact with rigid obstacles, fixed or translating along a path: the arithmetic of the term, in one place, and the stand-alone node kernels.
//   E_c = sum_o sum_i (k_o w_i / 2) p^2,  p = min(0, phi_o(x_i)),  x_i = X_i + u_i
//   g_i = sum_o k_o w_i p n                                  n = grad phi_o(x_i)
//   B_i = sum_o k_o w_i ([phi_o < 0] n n^T + c (I - n n^T))    c = -p / |y| for the cavity, 0 otherwise (max-PSD of p Hess phi)
// Every kernel that forms r(u), K(u) x, the diagonal or the stored energy with the term calls contact_force / contact_apply /
// contact_diagonal / contact_energy below: the node passes of the tiles (vector_tiles.hip) in the same visit that sums the node's
// partials, the routes off the tiles through the stand-alone kernels at the end of this file (engine_contact.hip launches them).
// The table travels BY VALUE in the kernel arguments: it is the same for every lane, so it stays in scalar registers; count == 0 is "off"
// and the only thing such a kernel reads of it.
//
// Coulomb friction, lagged and smoothed (Li et al., "Incremental Potential Contact", 2020, section 5): with the normal force and the tangent
// plane frozen at a lag position xbar_i,
//   nbar = grad phi_o(xbar_i),  P = I - nbar nbar^T,  lam = k_o w_i max(0, -phi_o(xbar_i)),  s = P d_i,  y = |s|
//   D   = sum_o sum_i mu_o lam f0(y)                   f0 = -y^3 / (3 eps^2) + y^2 / eps + eps / 3  (y < eps),  y  otherwise
//   q_i = sum_o mu_o lam c1 s                          c1 = 2 / eps - y / eps^2  (y < eps),  1 / y  otherwise
//   H_i = sum_o mu_o lam (c1 P - c2 s s^T)             c2 = 1 / (eps^2 y)  (0 < y < eps),  0  (y == 0),  1 / y^3  otherwise
// q is the gradient of the convex D and H_i its symmetric positive semi-definite Hessian, with xbar frozen.  The slip source: xbar_i = X_i +
// ubar_i and d_i = u_i - ubar_i (the solvers and the implicit integrators; ubar null: zero), or, with slip_v set, xbar_i = X_i + u_i and
// d_i = slip_dt v_i (central differences: the lag state is the current position, the slip that of the half-step velocity).  An obstacle
// that moves along a path (fh_set_obstacle_paths) carries its displacement over the lag interval, c_o: the slip is s = P (d_i - c_o).  An obstacle with
// mu_o == 0, a node out of contact at xbar or at the centre of a ball or cavity gets nothing.  `friction` is set exactly when some
// mu_o > 0: with it clear no lane executes or loads anything of the term.  friction_force / friction_apply / friction_diagonal /
// friction_block / friction_potential are called wherever their contact_* twins are.
//
// FH_OBSTACLE_GRID: phi is the bi- / trilinear interpolant of a signed distance sampled on a regular grid (fh_sdf_grid_create; sdf_grid_eval
// below is the whole arithmetic).  Outside the box of the samples the obstacle does not exist for a node: phi = +infinity, no gradient.
// Inside, m = grad phi is not a unit vector: with gn = |m|, g = k w p m, B = k w [phi < 0] m m^T (Gauss-Newton: p Hess phi has a zero
// diagonal and is indefinite, so it is dropped as the ball's curvature is) and, in friction, nbar = m / gn and lam = k w max(0, -phi) gn
// at the lag position.  The three analytic kinds execute what they executed before the kind existed: every difference is behind a branch
// on the kind, and behind the template flag G (contact_eval) that the node passes of the tiles clear while no grid stands.
//
// Augmented Lagrangian (fh_set_contact_multipliers, fh_contact_multiplier_update): a multiplier per obstacle and node, kept as a LENGTH
// s_oi >= 0 that stands for the force lam_oi = k_o w_i s_oi (no division on the device, w_i = 0 is harmless).  With
//   phi_eff = phi_o(x_i) - s_oi,  p = min(0, phi_eff)
// everything above is formed from phi_eff where it was formed from phi: g = k w p n, B with [phi_eff < 0] and c = -p / |y|, the friction
// bound lam = k w max(0, -phi_eff(xbar)) with the CURRENT s_oi, and E_c = sum (k w / 2) (p^2 - s^2).  g is the gradient of E_c with s frozen.
// contact_gap stays the geometric min_o phi_o.  The update s <- max(0, s - phi_o(x_i)) is k_contact_multiplier_update.  The shift sits in
// contact_visit / friction_visit behind the template flag A, which the node passes of the tiles clear while no multipliers stand
// (ContactTable::mult null): such an instantiation is the kernel it was before the flag existed.  With A set and every s = 0 the
// arithmetic is phi - 0.0 and e - 0.0: the same bits.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fenris_hip.h"
#include "device_common.hpp"

namespace fenris_hip {

struct ContactObstacle {
    double p[3];      // a point of the plane / the centre / the position of sample (0, 0, 0), at the contact clock's current time (fh_set_obstacle_time)
    double n[3];      // half-space: the unit normal; grid: the spacings h
    union {
        double radius;
        const double* grid;   // grid: its block on the device (SDF_GRID_HEADER doubles that hold the three sample counts as ints, then the samples, x fastest)
    };
    double k;
    int kind, pad_;
    double c[3];      // c_o = d_o(t) - d_o(t_lag): the obstacle's own displacement over the lag interval (zero without a path)
};
// (a grid reuses n[] and radius and keeps its counts with its samples: the entry is as large as before the kind existed, so a table of
// analytic obstacles is loaded as it was)
static_assert(sizeof(ContactObstacle) == 96, "ContactObstacle grew");
constexpr int SDF_GRID_HEADER = 2;

struct ContactTable {
    int count, dim;          // count == 0: no obstacles; dim: the geometric (= solution) dimension
    const double* X;         // [N][dim] vertices
    const double* u;         // [N][dim] displacement (null: zero)
    const double* w;         // [N] node weights (null: 1)
    ContactObstacle o[FH_MAX_OBSTACLES];
    // friction (fh_set_friction): the coefficients, the slip length, the slip source (see above)
    double mu[FH_MAX_OBSTACLES];
    const double* ubar;      // [N][dim] lag displacement (null: zero)
    const double* slip_v;    // [N][dim] velocity (null: the slip is u - ubar)
    double slip_dt;
    double eps;
    int friction, grids;     // friction != 0: some mu > 0; grids != 0: some obstacle is a grid
    const double* mult;      // [count][mult_stride] multiplier lengths s_oi (null: none stand)
    size_t mult_stride;      // >= N
};
inline ContactTable contact_off() {
    ContactTable t{};
    return t;
}
// the table travels in the kernel arguments beside the node pass's own (the largest: k_operator_from_partials, 96 bytes, and
// k_dynamics_from_partials with its DynStep; vector_tiles.hip holds both under NODE_PASS_ARG_BYTES): the whole block stays under the 4 KB
// a kernel's arguments may take
constexpr size_t NODE_PASS_ARG_BYTES = 512, KERNEL_ARG_LIMIT = 4096;
static_assert(sizeof(ContactTable) + NODE_PASS_ARG_BYTES <= KERNEL_ARG_LIMIT, "the contact table no longer fits the kernel arguments");

// A signed distance sampled on a regular grid (`block`: the counts cnt[3] as ints in SDF_GRID_HEADER doubles, then the samples; sample
// (ix, iy, iz) at values[(iz cnt[1] + iy) cnt[0] + ix], at origin + (ix h_0, iy h_1, iz h_2)), interpolated at x: with
// t_a = (x_a - origin_a) / h_a the point is inside iff 0 <= t_a <= cnt_a - 1 on every axis (a NaN is outside);
// i_a = min(floor(t_a), cnt_a - 2), f_a = t_a - i_a (the last face belongs to the last cell, f = 1); phi is the bi- / trilinear interpolant
// of the 4 / 8 corner samples of cell i at f and m its gradient in x (1 / h_a per axis included).  Returns whether x is inside; outside
// nothing is loaded and phi = +infinity, m = 0.  The corners are plain loads at compile-time offsets from one base index.  (On the host
// the samples cannot be read: every point is outside there.)
template <int D>
__host__ __device__ __forceinline__ bool sdf_grid_eval(const double* block, const double (&h)[3], const double (&origin)[3], const double (&x)[D],
                                                       double& phi, double (&m)[D]) {
    phi = HUGE_VAL;
#pragma unroll
    for (int a = 0; a < D; ++a) m[a] = 0.0;
#ifdef __HIP_DEVICE_COMPILE__
    const int* header = reinterpret_cast<const int*>(block);   // (the same address in every lane: the counts go to scalar registers)
    int cnt[D];
#pragma unroll
    for (int a = 0; a < D; ++a) cnt[a] = __builtin_amdgcn_readfirstlane(header[a]);
    const double* values = block + SDF_GRID_HEADER;
    double f[D];
    int i[D];
    bool inside = true;
#pragma unroll
    for (int a = 0; a < D; ++a) {
        const double t = (x[a] - origin[a]) / h[a];
        inside = inside && t >= 0.0 && t <= (double)(cnt[a] - 1);
        const int cell = inside ? (int)t : 0;   // (t >= 0: the conversion is the floor)
        i[a] = cell < cnt[a] - 2 ? cell : cnt[a] - 2;
        f[a] = t - (double)i[a];
    }
    if (!inside) return false;
    // (fewer than 2^31 samples: a sample index fits an int)
    int base = i[D - 1];
#pragma unroll
    for (int a = D - 2; a >= 0; --a) base = base * cnt[a] + i[a];
    const int stride[3] = {1, cnt[0], D == 3 ? cnt[0] * cnt[1] : 0};
    const double* cell = values + base;
    // the interpolant axis by axis: v[j] are the values left after the axes before `a` were interpolated, dv[b][j] their derivatives in
    // f_b; all indices are compile-time constants, the arrays live in registers
    double v[1 << D], dv[D][1 << D];
#pragma unroll
    for (int q = 0; q < (1 << D); ++q) {
        int at = 0;
#pragma unroll
        for (int a = 0; a < D; ++a)
            if (q >> a & 1) at += stride[a];
        v[q] = cell[at];
    }
#pragma unroll
    for (int a = 0; a < D; ++a) {
#pragma unroll
        for (int j = 0; j < (1 << (D - 1 - a)); ++j) {
            const double lo = v[2 * j], diff = v[2 * j + 1] - lo;
#pragma unroll
            for (int b = 0; b < a; ++b) dv[b][j] = dv[b][2 * j] + f[a] * (dv[b][2 * j + 1] - dv[b][2 * j]);
            dv[a][j] = diff;
            v[j] = lo + f[a] * diff;
        }
    }
    const double s = v[0];
    double ds[D];
#pragma unroll
    for (int a = 0; a < D; ++a) ds[a] = dv[a][0];
    phi = s;
#pragma unroll
    for (int a = 0; a < D; ++a) m[a] = ds[a] / h[a];
    return true;
#else
    (void)block, (void)h, (void)origin, (void)x;
    return false;
#endif
}

// phi, n = grad phi (has_n false: the centre of a ball or cavity, where the gradient does not exist; a grid: outside its box or on a flat
// spot) and 1 / |y| (0 for the half-space and the grid).  A grid hands back n = m, NOT normalised, and gn = |m|; the other kinds leave gn alone.
// G: whether the table may hold a grid (ContactTable::grids).  With G false the grid branch is not compiled: a kernel instantiated so is,
// instruction for instruction and register for register, the kernel of the three analytic kinds alone, and the node passes of the tiles
// launch that instantiation whenever no grid stands (a grid's 8 values in flight would otherwise set the register count of every launch).
template <int D, bool G = true>
__host__ __device__ __forceinline__ void contact_eval(const ContactObstacle& ob, const double (&x)[D], double& phi, double (&n)[D], bool& has_n,
                                                      double& inv_r, double& gn) {
    if (G && ob.kind == FH_OBSTACLE_GRID) {
        sdf_grid_eval<D>(ob.grid, ob.n, ob.p, x, phi, n);
        double m2 = 0.0;
#pragma unroll
        for (int c = 0; c < D; ++c) m2 += n[c] * n[c];
        gn = sqrt(m2);
        has_n = gn > 0.0;
        inv_r = 0.0;
        return;
    }
    if (ob.kind == FH_OBSTACLE_HALF_SPACE) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < D; ++c) {
            n[c] = ob.n[c];
            s += (x[c] - ob.p[c]) * ob.n[c];
        }
        phi = s;
        has_n = true;
        inv_r = 0.0;
        return;
    }
    double y[D], r2 = 0.0;
#pragma unroll
    for (int c = 0; c < D; ++c) {
        y[c] = x[c] - ob.p[c];
        r2 += y[c] * y[c];
    }
    const double r = sqrt(r2);
    const double sign = ob.kind == FH_OBSTACLE_BALL ? 1.0 : -1.0;
    phi = sign * (r - ob.radius);
    has_n = r > 0.0;
    inv_r = has_n ? 1.0 / r : 0.0;
#pragma unroll
    for (int c = 0; c < D; ++c) n[c] = has_n ? sign * y[c] * inv_r : 0.0;
}

// f(k w, phi, n, has_n, c) for every obstacle at node `node`, in the table's order (c: the coefficient of I - n n^T in B); only >= 0: that
// obstacle alone (the resultants).  A grid hands over n = m = grad phi as it is: k w p n and k w n n^T are its g and B, with c = 0
// A: whether multipliers may stand (ct.mult): phi handed to f is then phi_eff = phi - s_oi, and s_oi itself the last argument (0 without)
template <int D, bool G = true, bool A = true, class F>
__host__ __device__ __forceinline__ void contact_visit(const ContactTable& ct, int node, F&& f, int only = -1) {
    double x[D];
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = ct.X[(size_t)node * D + c] + (ct.u ? ct.u[(size_t)node * D + c] : 0.0);
    const double w = ct.w ? ct.w[node] : 1.0;
    for (int o = only < 0 ? 0 : only; o < (only < 0 ? ct.count : only + 1); ++o) {
        const ContactObstacle& ob = ct.o[o];
        double phi, n[D], inv_r, gn;
        bool has_n;
        contact_eval<D, G>(ob, x, phi, n, has_n, inv_r, gn);
        double sm = 0.0;
        if constexpr (A) {
            if (ct.mult) sm = ct.mult[(size_t)o * ct.mult_stride + node];
            phi -= sm;
        }
        const double p = phi < 0.0 ? phi : 0.0;
        f(ob.k * w, phi, n, has_n, ob.kind == FH_OBSTACLE_CAVITY ? -p * inv_r : 0.0, sm);
    }
}

// g[] += g_i
template <int D, bool G = true, bool A = true>
__host__ __device__ __forceinline__ void contact_force(const ContactTable& ct, int node, double (&g)[D]) {
    double s[D];
#pragma unroll
    for (int c = 0; c < D; ++c) s[c] = 0.0;
    contact_visit<D, G, A>(ct, node, [&](double kw, double phi, const double (&n)[D], bool has_n, double, double) {
        if (!(phi < 0.0) || !has_n) return;
        const double kp = kw * phi;
#pragma unroll
        for (int c = 0; c < D; ++c) s[c] += kp * n[c];
    });
#pragma unroll
    for (int c = 0; c < D; ++c) g[c] += s[c];
}

// y[] += scale B_i v
template <int D, bool G = true, bool A = true>
__host__ __device__ __forceinline__ void contact_apply(const ContactTable& ct, int node, const double (&v)[D], double scale, double (&y)[D]) {
    double s[D];
#pragma unroll
    for (int c = 0; c < D; ++c) s[c] = 0.0;
    contact_visit<D, G, A>(ct, node, [&](double kw, double phi, const double (&n)[D], bool has_n, double cc, double) {
        if (!(phi < 0.0) || !has_n) return;
        double nv = 0.0;
#pragma unroll
        for (int c = 0; c < D; ++c) nv += n[c] * v[c];
#pragma unroll
        for (int c = 0; c < D; ++c) s[c] += kw * (n[c] * nv + cc * (v[c] - n[c] * nv));
    });
#pragma unroll
    for (int c = 0; c < D; ++c) y[c] += scale * s[c];
}

// B[][] += B_i
template <int D, bool G = true, bool A = true>
__host__ __device__ __forceinline__ void contact_block(const ContactTable& ct, int node, double (&B)[D][D]) {
    contact_visit<D, G, A>(ct, node, [&](double kw, double phi, const double (&n)[D], bool has_n, double cc, double) {
        if (!(phi < 0.0) || !has_n) return;
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
            for (int b = 0; b < D; ++b) B[a][b] += kw * (n[a] * n[b] + cc * ((a == b ? 1.0 : 0.0) - n[a] * n[b]));
    });
}

// d[] += diag B_i
template <int D, bool G = true, bool A = true>
__host__ __device__ __forceinline__ void contact_diagonal(const ContactTable& ct, int node, double (&d)[D]) {
    contact_visit<D, G, A>(ct, node, [&](double kw, double phi, const double (&n)[D], bool has_n, double cc, double) {
        if (!(phi < 0.0) || !has_n) return;
#pragma unroll
        for (int c = 0; c < D; ++c) d[c] += kw * (n[c] * n[c] + cc * (1.0 - n[c] * n[c]));
    });
}

// the node's share of E_c, and min_o phi_o
template <int D, bool G = true, bool A = true>
__host__ __device__ __forceinline__ double contact_energy(const ContactTable& ct, int node) {
    double e = 0.0;
    contact_visit<D, G, A>(ct, node, [&](double kw, double phi, const double (&)[D], bool, double, double sm) {
        if (phi < 0.0) e += 0.5 * kw * phi * phi;
        if constexpr (A) e -= 0.5 * kw * sm * sm;   // (k w / 2) (p^2 - s^2); s = 0: e - 0.0
    });
    return e;
}
// (the geometric distance: never shifted by a multiplier)
template <int D, bool G = true>
__host__ __device__ __forceinline__ double contact_gap(const ContactTable& ct, int node) {
    double g = HUGE_VAL;
    contact_visit<D, G, false>(ct, node, [&](double, double phi, const double (&)[D], bool, double, double) { g = phi < g ? phi : g; });
    return g;
}

// f(mu lam, nbar, s, y, c1, c2) for every obstacle with mu > 0 that node `node` touches at its lag position, in the table's order.  A moving
// obstacle (c_o != 0): the slip is taken relative to the obstacle, s = P (d_i - c_o), and with the lag displacement as the slip source the
// obstacle stands at its lag position p - c_o; with slip_v the lag configuration is the current one, obstacle included.
// With A the node is in contact at xbar iff phi_eff(xbar) = phi(xbar) - s_oi < 0, s_oi the multiplier as it stands now.
template <int D, bool G = true, bool A = true, class F>
__host__ __device__ __forceinline__ void friction_visit(const ContactTable& ct, int node, F&& f, int only = -1) {
    double x[D], d[D];
#pragma unroll
    for (int c = 0; c < D; ++c) {
        const size_t i = (size_t)node * D + c;
        const double u = ct.u ? ct.u[i] : 0.0;
        if (ct.slip_v) {
            x[c] = ct.X[i] + u;
            d[c] = ct.slip_dt * ct.slip_v[i];
        } else {
            const double ub = ct.ubar ? ct.ubar[i] : 0.0;
            x[c] = ct.X[i] + ub;
            d[c] = u - ub;
        }
    }
    const double w = ct.w ? ct.w[node] : 1.0;
    const double inv_eps = 1.0 / ct.eps;
    for (int o = only < 0 ? 0 : only; o < (only < 0 ? ct.count : only + 1); ++o) {
        if (!(ct.mu[o] > 0.0)) continue;
        ContactObstacle ob = ct.o[o];
        double rel[D];
#pragma unroll
        for (int c = 0; c < D; ++c) {
            rel[c] = d[c] - ob.c[c];
            if (!ct.slip_v) ob.p[c] -= ob.c[c];
        }
        double phi, n[D], inv_r, gn;
        bool has_n;
        contact_eval<D, G>(ob, x, phi, n, has_n, inv_r, gn);
        if constexpr (A) {
            if (ct.mult) phi -= ct.mult[(size_t)o * ct.mult_stride + node];
        }
        if (!(phi < 0.0) || !has_n) continue;
        double kw = ob.k * w;
        if (G && ob.kind == FH_OBSTACLE_GRID) {   // nbar = m / |m|, and the normal force k w |phi| |m| bounds |q|
#pragma unroll
            for (int c = 0; c < D; ++c) n[c] /= gn;
            kw *= gn;
        }
        double nd = 0.0;
#pragma unroll
        for (int c = 0; c < D; ++c) nd += n[c] * rel[c];
        double s[D], y2 = 0.0;
#pragma unroll
        for (int c = 0; c < D; ++c) {
            s[c] = rel[c] - n[c] * nd;
            y2 += s[c] * s[c];
        }
        const double y = sqrt(y2);
        double c1, c2;
        if (y < ct.eps) {   // (never a division by y here: y == 0 gives q = 0 and c2 = 0)
            c1 = 2.0 * inv_eps - y * inv_eps * inv_eps;
            c2 = y > 0.0 ? inv_eps * inv_eps / y : 0.0;
        } else {
            c1 = 1.0 / y;
            c2 = c1 * c1 * c1;
        }
        f(ct.mu[o] * (kw * -phi), n, s, y, c1, c2);
    }
}

// q[] += q_i
template <int D, bool G = true, bool A = true>
__host__ __device__ __forceinline__ void friction_force(const ContactTable& ct, int node, double (&q)[D]) {
    double t[D];
#pragma unroll
    for (int c = 0; c < D; ++c) t[c] = 0.0;
    friction_visit<D, G, A>(ct, node, [&](double ml, const double (&)[D], const double (&s)[D], double, double c1, double) {
        const double m1 = ml * c1;
#pragma unroll
        for (int c = 0; c < D; ++c) t[c] += m1 * s[c];
    });
#pragma unroll
    for (int c = 0; c < D; ++c) q[c] += t[c];
}

// y[] += scale H_i v
template <int D, bool G = true, bool A = true>
__host__ __device__ __forceinline__ void friction_apply(const ContactTable& ct, int node, const double (&v)[D], double scale, double (&y)[D]) {
    double t[D];
#pragma unroll
    for (int c = 0; c < D; ++c) t[c] = 0.0;
    friction_visit<D, G, A>(ct, node, [&](double ml, const double (&n)[D], const double (&s)[D], double, double c1, double c2) {
        double nv = 0.0, sv = 0.0;
#pragma unroll
        for (int c = 0; c < D; ++c) {
            nv += n[c] * v[c];
            sv += s[c] * v[c];
        }
#pragma unroll
        for (int c = 0; c < D; ++c) t[c] += ml * (c1 * (v[c] - n[c] * nv) - c2 * sv * s[c]);
    });
#pragma unroll
    for (int c = 0; c < D; ++c) y[c] += scale * t[c];
}

// B[][] += H_i
template <int D, bool G = true, bool A = true>
__host__ __device__ __forceinline__ void friction_block(const ContactTable& ct, int node, double (&B)[D][D]) {
    friction_visit<D, G, A>(ct, node, [&](double ml, const double (&n)[D], const double (&s)[D], double, double c1, double c2) {
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
            for (int b = 0; b < D; ++b) {   // (the upper triangle's expression on both sides: symmetric to the bit, the diagonal friction_diagonal's)
                const int lo = a < b ? a : b, hi = a < b ? b : a;
                B[a][b] += ml * (c1 * ((a == b ? 1.0 : 0.0) - n[lo] * n[hi]) - c2 * s[lo] * s[hi]);
            }
    });
}

// d[] += diag H_i
template <int D, bool G = true, bool A = true>
__host__ __device__ __forceinline__ void friction_diagonal(const ContactTable& ct, int node, double (&d)[D]) {
    friction_visit<D, G, A>(ct, node, [&](double ml, const double (&n)[D], const double (&s)[D], double, double c1, double c2) {
#pragma unroll
        for (int c = 0; c < D; ++c) d[c] += ml * (c1 * (1.0 - n[c] * n[c]) - c2 * s[c] * s[c]);
    });
}

// the node's share of D
template <int D, bool G = true, bool A = true>
__host__ __device__ __forceinline__ double friction_potential(const ContactTable& ct, int node) {
    double e = 0.0;
    friction_visit<D, G, A>(ct, node, [&](double ml, const double (&)[D], const double (&)[D], double y, double, double) {
        const double eps = ct.eps;
        e += ml * (y < eps ? -y * y * y / (3.0 * eps * eps) + y * y / eps + eps / 3.0 : y);
    });
    return e;
}

#ifdef __HIPCC__
// fh_sdf_grid_sample_dev: the interpolant alone at m points, one lane per point, grid-stride; outside: phi = +infinity, a zero gradient
template <int D>
__global__ void __launch_bounds__(256) k_sdf_grid_sample(const ContactObstacle ob, const double* points, unsigned long long count, double* phi_out,
                                                         double* grad_out) {
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (unsigned long long)gridDim.x * 256) {
        double x[D], phi, m[D];
#pragma unroll
        for (int c = 0; c < D; ++c) x[c] = points[i * D + c];
        sdf_grid_eval<D>(ob.grid, ob.n, ob.p, x, phi, m);
        phi_out[i] = phi;
        if (grad_out) {
#pragma unroll
            for (int c = 0; c < D; ++c) grad_out[i * D + c] = m[c];
        }
    }
}

// ---- the stand-alone node kernels: one thread per node

// per-workgroup partials of E_c in a fixed tree; the caller sums them in index order (k_sum_partial_ranges / sum_partials)
template <int D>
__global__ void __launch_bounds__(256) k_contact_energy(const ContactTable ct, int num_nodes, double* partial) {
    __shared__ double red[4];
    const int node = blockIdx.x * 256 + threadIdx.x;
    const double e = node < num_nodes ? contact_energy<D>(ct, node) : 0.0;
    const double tot = block_sum_256(e, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// ... and of the friction potential D, the same way
template <int D>
__global__ void __launch_bounds__(256) k_friction_potential(const ContactTable ct, int num_nodes, double* partial) {
    __shared__ double red[4];
    const int node = blockIdx.x * 256 + threadIdx.x;
    const double e = node < num_nodes && ct.friction ? friction_potential<D>(ct, node) : 0.0;
    const double tot = block_sum_256(e, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// out += g (parts & 1) + q (parts & 2, while friction is set)
template <int D>
__global__ void __launch_bounds__(256) k_contact_force(const ContactTable ct, int num_nodes, double* out, int parts) {
    const int node = blockIdx.x * 256 + threadIdx.x;
    if (node >= num_nodes) return;
    double g[D];
#pragma unroll
    for (int c = 0; c < D; ++c) g[c] = out[(size_t)node * D + c];
    if (parts & 1) contact_force<D>(ct, node, g);
    if ((parts & 2) && ct.friction) friction_force<D>(ct, node, g);
#pragma unroll
    for (int c = 0; c < D; ++c) out[(size_t)node * D + c] = g[c];
}

template <int D>
__global__ void __launch_bounds__(256) k_contact_gap(const ContactTable ct, int num_nodes, double* gap) {
    const int node = blockIdx.x * 256 + threadIdx.x;
    if (node < num_nodes) gap[node] = contact_gap<D>(ct, node);
}

// y += (B + H) x 2^-e (xbits: mf_exponent of the operand the element pass of the map saw, may be null: the pass that finishes y multiplies by 2^e);
// the held components of x (dmask, may be null) read as zero, as the element pass read them
template <int D>
__global__ void __launch_bounds__(256) k_contact_apply(const ContactTable ct, int num_nodes, const double* x, const unsigned char* dmask,
                                                       const unsigned long long* xbits, double* y) {
    const int node = blockIdx.x * 256 + threadIdx.x;
    if (node >= num_nodes) return;
    const int ex = mf_exponent(xbits);
    const unsigned fixed = node_dmask(dmask, node);
    double v[D], s[D];
#pragma unroll
    for (int c = 0; c < D; ++c) {
        v[c] = comp_fixed(fixed, c) ? 0.0 : x[(size_t)node * D + c];
        s[c] = 0.0;
    }
    contact_apply<D>(ct, node, v, 1.0, s);
    if (ct.friction) friction_apply<D>(ct, node, v, 1.0, s);
#pragma unroll
    for (int c = 0; c < D; ++c) y[(size_t)node * D + c] += ldexp(s[c], -ex);
}

// diag += diag (B + H)
template <int D>
__global__ void __launch_bounds__(256) k_contact_diagonal(const ContactTable ct, int num_nodes, double* diag) {
    const int node = blockIdx.x * 256 + threadIdx.x;
    if (node >= num_nodes) return;
    double d[D];
#pragma unroll
    for (int c = 0; c < D; ++c) d[c] = diag[(size_t)node * D + c];
    contact_diagonal<D>(ct, node, d);
    if (ct.friction) friction_diagonal<D>(ct, node, d);
#pragma unroll
    for (int c = 0; c < D; ++c) diag[(size_t)node * D + c] = d[c];
}

// B_i + H_i added to the diagonal node block of block row `node` of the pattern's CSR values (row S i + a holds cnt blocks of S entries; the
// columns of a row are sorted: a binary search finds the node's own)
template <int D>
__global__ void __launch_bounds__(256) k_contact_csr(const ContactTable ct, int num_nodes, const unsigned* noff, const unsigned* ncols,
                                                     double* vals) {
    const int node = blockIdx.x * 256 + threadIdx.x;
    if (node >= num_nodes) return;
    const unsigned r0 = noff[node], cnt = noff[node + 1] - r0;
    unsigned lo = 0, hi = cnt;
    while (lo < hi) {
        const unsigned mid = (lo + hi) / 2;
        if (ncols[r0 + mid] < (unsigned)node) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= cnt || ncols[r0 + lo] != (unsigned)node) return;   // (a pattern always holds the diagonal block)
    double B[D][D];
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b) B[a][b] = 0.0;
    contact_block<D>(ct, node, B);
    if (ct.friction) friction_block<D>(ct, node, B);
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b) vals[(size_t)D * D * r0 + (size_t)a * D * cnt + (size_t)D * lo + b] += B[a][b];
}

// the force resultants per obstacle (fh_contact_resultants): R_o = sum_i k_o w_i p n, obstacle o's share of g, and Q_o = sum_i mu_o lam c1 s,
// its share of q (zeros while friction is clear).  One thread per node; per obstacle and component the lanes of a wavefront are summed by
// xor-shuffles (the tree of block_sum_256), the wavefront sums go to LDS, and after ONE barrier thread k < 6 count adds the four of entry k
// as (w0 + w1) + (w2 + w3) and writes it: row blockIdx.x of `partial` holds 6 count doubles, [o][R_x R_y R_z Q_x Q_y Q_z] (2-D: the third
// components are zero).  The caller sums the rows in index order (sum_partials): no atomics, two calls give the same bits.
template <int D>
__global__ void __launch_bounds__(256) k_contact_resultants(const ContactTable ct, int num_nodes, double* partial) {
    __shared__ double red[FH_MAX_OBSTACLES * 6][4];
    const int node = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = 0; o < ct.count; ++o) {   // (count is uniform: every lane takes part in every shuffle)
        double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (node < num_nodes) {
            contact_visit<D>(ct, node, [&](double kw, double phi, const double (&n)[D], bool has_n, double, double) {
                if (!(phi < 0.0) || !has_n) return;
                const double kp = kw * phi;
#pragma unroll
                for (int c = 0; c < D; ++c) v[c] += kp * n[c];
            }, o);
            if (ct.friction)
                friction_visit<D>(ct, node, [&](double ml, const double (&)[D], const double (&s)[D], double, double c1, double) {
                    const double m1 = ml * c1;
#pragma unroll
                    for (int c = 0; c < D; ++c) v[3 + c] += m1 * s[c];
                }, o);
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            double t = v[k];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off);
            if (lane == 0) red[o * 6 + k][wave] = t;
        }
    }
    __syncthreads();
    const int K = 6 * ct.count;
    if ((int)threadIdx.x < K)
        partial[(size_t)blockIdx.x * K + threadIdx.x] = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
}

// ---- augmented Lagrangian: the multiplier update and the forces the multipliers stand for

// max of v >= 0 over the lanes of a wavefront (xor-shuffles: every lane ends with it)
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double t = __shfl_xor(v, off);
        v = t > v ? t : v;
    }
    return v;
}

// fh_contact_multiplier_update: s_oi <- max(0, s_oi - phi_o(x_i)) in place, one thread per node, the obstacles in the table's order
// (phi = +infinity outside a grid's box: 0).  `ct` is the table WITHOUT multipliers (phi is the geometric distance); mult: [count][stride],
// read and written by this lane alone.  skip (may be null): a byte per node, nonzero: the node keeps s = 0 and stays out of the
// statistics.  Row blockIdx.x of `partial` holds 4 doubles over the workgroup's counted (node, obstacle) pairs: max |s_new - s_old|,
// max max(0, -phi), the number with s_new > 0, max lam = k w s_new (a grid: times |grad phi|).  The lanes of a wavefront are combined by
// xor-shuffles, the four wavefronts through LDS in index order after ONE barrier; the caller combines the rows in index order.  No
// atomics: equal input gives equal bits.
template <int D>
__global__ void __launch_bounds__(256) k_contact_multiplier_update(const ContactTable ct, int num_nodes, double* mult, size_t stride,
                                                                   const unsigned char* skip, double* partial) {
    __shared__ double red[4][4];
    const int node = blockIdx.x * 256 + threadIdx.x;
    double change = 0.0, pen = 0.0, active = 0.0, lam = 0.0;
    if (node < num_nodes) {
        double x[D];
#pragma unroll
        for (int c = 0; c < D; ++c) x[c] = ct.X[(size_t)node * D + c] + (ct.u ? ct.u[(size_t)node * D + c] : 0.0);
        const double w = ct.w ? ct.w[node] : 1.0;
        const bool held = skip && skip[node];
        for (int o = 0; o < ct.count; ++o) {
            const ContactObstacle& ob = ct.o[o];
            double phi, n[D], inv_r, gn = 1.0;
            bool has_n;
            contact_eval<D>(ob, x, phi, n, has_n, inv_r, gn);
            double* at = mult + (size_t)o * stride + node;
            if (held) {
                *at = 0.0;
                continue;
            }
            const double s_old = *at, t = s_old - phi;
            const double s_new = t > 0.0 ? t : 0.0;
            *at = s_new;
            const double dc = fabs(s_new - s_old), dp = phi < 0.0 ? -phi : 0.0;
            const double l = ob.k * w * s_new * (ob.kind == FH_OBSTACLE_GRID ? gn : 1.0);
            change = dc > change ? dc : change;
            pen = dp > pen ? dp : pen;
            active += s_new > 0.0 ? 1.0 : 0.0;
            lam = l > lam ? l : lam;
        }
    }
    change = wave_max(change);
    pen = wave_max(pen);
    lam = wave_max(lam);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) active += __shfl_xor(active, off);   // (whole numbers: exact)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[0][wave] = change;
        red[1][wave] = pen;
        red[2][wave] = active;
        red[3][wave] = lam;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const double* r = red[threadIdx.x];
        double v;
        if (threadIdx.x == 2) v = (r[0] + r[1]) + (r[2] + r[3]);
        else {
            const double a = r[0] > r[1] ? r[0] : r[1], b = r[2] > r[3] ? r[2] : r[3];
            v = a > b ? a : b;
        }
        partial[(size_t)blockIdx.x * 4 + threadIdx.x] = v;
    }
}

// fh_contact_multiplier_forces_dev: lam[o][i] = k_o w_i s_oi, for a grid times |grad phi| at the node's current position (0 outside its box)
template <int D>
__global__ void __launch_bounds__(256) k_contact_multiplier_forces(const ContactTable ct, int num_nodes, double* lam) {
    const int node = blockIdx.x * 256 + threadIdx.x;
    if (node >= num_nodes) return;
    double x[D];
#pragma unroll
    for (int c = 0; c < D; ++c) x[c] = ct.X[(size_t)node * D + c] + (ct.u ? ct.u[(size_t)node * D + c] : 0.0);
    const double w = ct.w ? ct.w[node] : 1.0;
    for (int o = 0; o < ct.count; ++o) {
        const ContactObstacle& ob = ct.o[o];
        const double s = ct.mult ? ct.mult[(size_t)o * ct.mult_stride + node] : 0.0;
        double f = ob.k * w * s;
        if (ob.kind == FH_OBSTACLE_GRID) {
            double phi, n[D], inv_r, gn = 0.0;
            bool has_n;
            contact_eval<D>(ob, x, phi, n, has_n, inv_r, gn);
            f *= gn;
        }
        lam[(size_t)o * num_nodes + node] = f;
    }
}
#endif

}  // namespace fenris_hip
