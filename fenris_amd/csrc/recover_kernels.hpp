// Recovery of the quantities a user reads off a solved field (engine_recover.hip): displacement gradient, strain, operator (first
// Piola-Kirchhoff) stress, Cauchy stress, von Mises stress, energy density and element measure -- per (element, quadrature point), as the
// measure-weighted element mean, and as the volume-weighted patch average at the nodes.  A pure per-point map on what the residual's
// element pass already forms (grad u = J^-T sum_n ghat_n u_n^T, element_pass.hpp) followed by material_point (material.hpp), so nothing leaves
// the device.
//
//  * k_recover_elements<EK, OP, QUANTITY, FH_AT_ELEMENTS>, the four iso-parametric kinds: ONE THREAD PER ELEMENT in the register-resident
//    form of element_pass.hpp -- vertex coordinates and u of the element in registers, the tables through scalar loads (ep_const), J, its
//    inverse and grad u per point in registers, sum_q w |det J| v_q and sum_q w |det J| accumulated in point order.  Writes the mean and / or
//    V_e: one coalesced row per lane.
//  * k_recover_elements<EK, OP, QUANTITY, FH_AT_POINTS>, all ten kinds: ONE THREAD PER (ELEMENT, POINT).  Geometry from the NG vertex nodes,
//    the field from all n nodes; every accumulator is indexed at compile time (no private array meets a run-time index: no scratch).  Lane t
//    writes row t of the (E nq) x ncomp output, so a wavefront's stores are one contiguous piece.  With `measure` given it also leaves
//    w |det J| per point, and k_recover_means sums the points of an element in point order: the element mean of the quadratic kinds.
//  * k_recover_nodes<NCOMP>: one thread per node walks the node's adjacency row in ascending element order,
//    out_n = sum V_e mean_e / sum V_e over its active elements.  No atomics anywhere: two calls agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include "device_common.hpp"
#include "element_pass.hpp"
#include "material.hpp"
#include "small_ops.hpp"

namespace fenris_hip {

struct RecoverArgs {
    const unsigned char* active;   // E flags of fh_set_active_elements, or null
    double* points;                // (E nq) x ncomp, or null
    double* measure;               // E nq: w |det J| of every point, or null
    double* mean;                  // E x ncomp, or null
    double* volume;                // E, or null
};

// components of a quantity for an operator in D dimensions
template <int OP, int D, int Q>
struct RecoverComp {
    static constexpr int S = OpT<OP, D>::S;
    static constexpr int NC = Q == FH_RECOVER_GRAD_U ? D * S
                            : (Q == FH_RECOVER_STRAIN || Q == FH_RECOVER_STRESS_CAUCHY) ? D * D
                            : Q == FH_RECOVER_STRESS_PK1 ? S * D : 1;
};
// the (operator, quantity) pairs that exist: Laplace has a gradient, a flux and an energy density; the measure needs no operator and
// is instantiated once, under FH_LAPLACE
template <int OP, int Q>
constexpr bool recover_defined = Q == FH_RECOVER_VOLUME ? OP == FH_LAPLACE
                               : OP == FH_LAPLACE ? (Q == FH_RECOVER_GRAD_U || Q == FH_RECOVER_STRESS_PK1 || Q == FH_RECOVER_ENERGY_DENSITY)
                               : true;

// the quantity's components v (row-major) of one point from grad u (gu[i][k] = d u_k / d x_i) and the point's Lame parameters
template <int OP, int D, int S, int Q>
__device__ __forceinline__ void recover_values(const double (&gu)[D][S], double mu, double lambda, double (&v)[RecoverComp<OP, D, Q>::NC]) {
    static_assert(recover_defined<OP, Q>, "no such quantity for this operator");
    if constexpr (Q == FH_RECOVER_VOLUME) {
        v[0] = 0.0;
    } else if constexpr (Q == FH_RECOVER_GRAD_U) {
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int k = 0; k < S; ++k) v[i * S + k] = gu[i][k];
    } else if constexpr (Q == FH_RECOVER_STRAIN) {
        if constexpr (OP == FH_LINEAR_ELASTIC) {   // sym(grad u)
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int j = 0; j < D; ++j) v[i * D + j] = 0.5 * (gu[i][j] + gu[j][i]);
        } else {   // Green-Lagrange (F^T F - I) / 2 with F = I + (grad u)^T  (fenris-solid/src/lib.rs:20-29)
            double F[D][D], E[D][D];
            deformation_gradient<D, S>(gu, F);
            green_strain<D>(F, E);
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int j = 0; j < D; ++j) v[i * D + j] = E[i][j];
        }
    } else if constexpr (Q == FH_RECOVER_ENERGY_DENSITY) {
        double P[S][D], psi;
        material_point<OP, D, S, EP_SCALAR>(gu, mu, lambda, P, psi);
        v[0] = psi;
    } else {
        double P[S][D], psi;
        material_point<OP, D, S, EP_VECTOR>(gu, mu, lambda, P, psi);
        if constexpr (Q == FH_RECOVER_STRESS_PK1) {
#pragma unroll
            for (int i = 0; i < S; ++i)
#pragma unroll
                for (int j = 0; j < D; ++j) v[i * D + j] = P[i][j];
        } else {
            double sg[D][D];   // Cauchy stress: P for LinearElastic, P F^T / det F for the hyperelastic materials (NaN when det F <= 0)
            if constexpr (OP == FH_LINEAR_ELASTIC) {
#pragma unroll
                for (int i = 0; i < D; ++i)
#pragma unroll
                    for (int j = 0; j < D; ++j) sg[i][j] = P[i][j];
            } else {
                double F[D][D];
                deformation_gradient<D, S>(gu, F);
                const double Jd = det_small<D>(F);
                const double rj = Jd <= 0.0 ? __builtin_nan("") : 1.0 / Jd;
#pragma unroll
                for (int i = 0; i < D; ++i)
#pragma unroll
                    for (int j = 0; j < D; ++j) {
                        double t = 0.0;
#pragma unroll
                        for (int k = 0; k < D; ++k) t = fma(P[i][k], F[j][k], t);
                        sg[i][j] = t * rj;
                    }
            }
            if constexpr (Q == FH_RECOVER_STRESS_CAUCHY) {
#pragma unroll
                for (int i = 0; i < D; ++i)
#pragma unroll
                    for (int j = 0; j < D; ++j) v[i * D + j] = sg[i][j];
            } else if constexpr (D == 2) {   // in-plane form: sqrt(sxx^2 - sxx syy + syy^2 + 3 sxy^2)
                v[0] = sqrt(sg[0][0] * sg[0][0] - sg[0][0] * sg[1][1] + sg[1][1] * sg[1][1] + 3.0 * (sg[0][1] * sg[0][1]));
            } else {                         // sqrt(3/2 dev : dev)
                const double m = (sg[0][0] + sg[1][1] + sg[2][2]) * (1.0 / 3.0);
                double dd = 0.0;
#pragma unroll
                for (int i = 0; i < D; ++i)
#pragma unroll
                    for (int j = 0; j < D; ++j) {
                        const double t = sg[i][j] - (i == j ? m : 0.0);
                        dd = fma(t, t, dd);
                    }
                v[0] = sqrt(1.5 * dd);
            }
        }
    }
}

// the quantities that come from the elastic part under a per-element expansion (material.hpp, Stretch): the stresses and the energy
// density.  The gradient and the strain stay the total ones.
template <int OP, int Q>
constexpr bool recover_expands = op_expands(OP) && (Q == FH_RECOVER_STRESS_PK1 || Q == FH_RECOVER_STRESS_CAUCHY || Q == FH_RECOVER_VON_MISES ||
                                                    Q == FH_RECOVER_ENERGY_DENSITY);
// recover_values of element e's point under its stretch (EX; gu is consumed): the first Piola-Kirchhoff stress theta^(d-1) P_0(gu_e) and the
// energy density theta^d psi_0(gu_e) per reference volume; the Cauchy stress P F^T / det F of the total F is the one of the elastic part
// alone (the powers of theta cancel), and so is von Mises'
template <int OP, int D, int S, int Q, bool EX>
__device__ __forceinline__ void recover_point(const KArgs& a, const long long e, double (&gu)[D][S], double mu, double lambda,
                                              double (&v)[RecoverComp<OP, D, Q>::NC]) {
    if constexpr (EX && recover_expands<OP, Q>) {
        const Stretch<OP, D> st = element_stretch<OP, D>(a, e);
        stretch_strain<OP, D, S>(st, gu);
        recover_values<OP, D, S, Q>(gu, mu, lambda, v);
        if constexpr (Q == FH_RECOVER_STRESS_PK1 && !Stretch<OP, D>::additive) {
#pragma unroll
            for (int c = 0; c < RecoverComp<OP, D, Q>::NC; ++c) v[c] *= st.sP;
        } else if constexpr (Q == FH_RECOVER_ENERGY_DENSITY && !Stretch<OP, D>::additive) {
            v[0] *= st.sPsi;
        }
    } else {
        recover_values<OP, D, S, Q>(gu, mu, lambda, v);
    }
}

// J -> |det J| and grad u = J^-T R.  det J == 0 exactly is reported like the residual reports it (elliptic.rs:401-404), the inverse is zero then.
template <int D, int S>
__device__ __forceinline__ double recover_grad_u(const KArgs& a, const long long e, const double (&J)[D][D], const double (&R)[D][S],
                                                 double (&gu)[D][S]) {
    double Ji[D][D];
    const double detJ = inverse_or_zeros(J, Ji, [&] { report_singular(a.status, e); });
    pull_back<D, S>(Ji, R, gu);
    return fabs(detJ);
}

// WHERE = FH_AT_ELEMENTS (Quad4, Tri3, Tet4, Hex8): one thread per element, mean and / or V_e.
// WHERE = FH_AT_POINTS (every kind): one thread per (element, point), the point's row and / or its measure.
// Masked elements write zeros.  EX: with the per-element expansion of a.theta (recover_point); EX = false is the kernel as it was.
template <int EK, int OP, int Q, int WHERE, bool EX = false>
__global__ void __launch_bounds__(256) k_recover_elements(const KArgs a, const RecoverArgs r) {
    using E = ElemT<EK>;
    constexpr int D = E::D, N = E::N, NG = E::NG, S = OpT<OP, D>::S, NC = RecoverComp<OP, D, Q>::NC;
    constexpr bool FIELD = Q != FH_RECOVER_VOLUME;
    static_assert(WHERE == FH_AT_POINTS || (WHERE == FH_AT_ELEMENTS && N == NG && N <= 8), "thread per element: small iso-parametric elements");
    if constexpr (WHERE == FH_AT_ELEMENTS) {
        const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
        if (e >= a.num_elements) return;
        if (r.active && !r.active[e]) {
            if (r.volume) r.volume[e] = 0.0;
            if (r.mean) {
#pragma unroll
                for (int c = 0; c < NC; ++c) r.mean[(size_t)e * NC + c] = 0.0;
            }
            return;
        }
        double X[N][D], U[FIELD ? N : 1][S];
#pragma unroll
        for (int n = 0; n < N; ++n) {
            const int nd = a.conn[(size_t)e * N + n];
#pragma unroll
            for (int i = 0; i < D; ++i) X[n][i] = a.verts[(size_t)nd * D + i];
            if constexpr (FIELD) {
#pragma unroll
                for (int k = 0; k < S; ++k) U[n][k] = a.u ? a.u[(size_t)nd * S + k] : 0.0;
            }
        }
        const double* par_e = a.rule_map ? a.rparams + (size_t)a.rule_map[e] * a.nq * 2 : nullptr;
        double acc[NC], vol = 0.0;
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] = 0.0;
        for (int q = 0; q < a.nq; ++q) {
            const ep_table G = ep_const(a.gref) + (size_t)q * N * D;   // uniform over the wavefront: scalar loads
            double J[D][D], R[D][S];
#pragma unroll
            for (int i = 0; i < D; ++i) {
#pragma unroll
                for (int j = 0; j < D; ++j) J[i][j] = 0.0;
#pragma unroll
                for (int k = 0; k < S; ++k) R[i][k] = 0.0;
            }
#pragma unroll
            for (int n = 0; n < N; ++n)
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    const double g = G[n * D + j];
#pragma unroll
                    for (int i = 0; i < D; ++i) J[i][j] = fma(X[n][i], g, J[i][j]);   // J = X G^T
                    if constexpr (FIELD) {
#pragma unroll
                        for (int k = 0; k < S; ++k) R[j][k] = fma(g, U[n][k], R[j][k]);   // sum_n ghat_n u_n^T
                    }
                }
            double gu[D][S];
            const double s = ep_const(a.qw)[q] * recover_grad_u<D, S>(a, e, J, R, gu);   // w |det J|
            vol += s;
            if constexpr (FIELD) {
                double mu, lambda;
                point_params<OP>(a, par_e, q, mu, lambda);
                double v[NC];
                recover_point<OP, D, S, Q, EX>(a, e, gu, mu, lambda, v);
#pragma unroll
                for (int c = 0; c < NC; ++c) acc[c] = fma(s, v[c], acc[c]);
            }
        }
        if (r.volume) r.volume[e] = vol;
        if (FIELD && r.mean) {
#pragma unroll
            for (int c = 0; c < NC; ++c) r.mean[(size_t)e * NC + c] = acc[c] / vol;
        }
    } else {
        const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
        if (t >= a.num_elements * a.nq) return;
        const long long e = t / a.nq;
        const int q = (int)(t - e * a.nq);
        if (r.active && !r.active[e]) {
            if (r.measure) r.measure[t] = 0.0;
            if (FIELD && r.points) {
#pragma unroll
                for (int c = 0; c < NC; ++c) r.points[(size_t)t * NC + c] = 0.0;
            }
            return;
        }
        const int* cn = a.conn + (size_t)e * N;
        const double* Gg = a.ggeom + (size_t)q * NG * D;
        double J[D][D], R[D][S];
#pragma unroll
        for (int i = 0; i < D; ++i) {
#pragma unroll
            for (int j = 0; j < D; ++j) J[i][j] = 0.0;
#pragma unroll
            for (int k = 0; k < S; ++k) R[i][k] = 0.0;
        }
#pragma unroll 4
        for (int n = 0; n < NG; ++n) {   // the geometry map: the vertex nodes (kind_geom)
            const double* x = a.verts + (size_t)cn[n] * D;
#pragma unroll
            for (int j = 0; j < D; ++j) {
                const double g = Gg[n * D + j];
#pragma unroll
                for (int i = 0; i < D; ++i) J[i][j] = fma(x[i], g, J[i][j]);
            }
        }
        if constexpr (FIELD) {
            const double* G = a.gref + (size_t)q * N * D;
            // (a few nodes at a time: with all the loads of a 27-node element in flight at once the lane took every register there is)
            constexpr int UNR = N <= 6 ? N : (N % 4 == 0 ? 4 : 3);
#pragma unroll UNR
            for (int n = 0; n < N; ++n) {   // the field: all nodes
                const size_t nd = (size_t)cn[n];
#pragma unroll
                for (int k = 0; k < S; ++k) {
                    const double un = a.u ? a.u[nd * S + k] : 0.0;
#pragma unroll
                    for (int j = 0; j < D; ++j) R[j][k] = fma(G[n * D + j], un, R[j][k]);
                }
            }
        }
        double gu[D][S];
        const double s = a.qw[q] * recover_grad_u<D, S>(a, e, J, R, gu);
        if (r.measure) r.measure[t] = s;
        if constexpr (FIELD) {
            if (r.points) {
                double mu = 0.0, lambda = 0.0;
                if (OP != FH_LAPLACE) {
                    const double* p = a.rule_map ? a.rparams + ((size_t)a.rule_map[e] * a.nq + q) * 2 : a.qparams + 2 * q;
                    mu = p[0];
                    lambda = p[1];
                }
                double v[NC];
                recover_point<OP, D, S, Q, EX>(a, e, gu, mu, lambda, v);
#pragma unroll
                for (int c = 0; c < NC; ++c) r.points[(size_t)t * NC + c] = v[c];
            }
        }
    }
}

// element means off the point rows: one thread per (element, component), sum_q s_q v_q / sum_q s_q in point order (s = w |det J|);
// c == 0 also writes V_e.  points null: the measure alone.
__global__ void __launch_bounds__(256) k_recover_means(long long E, int nq, int nc, const unsigned char* active, const double* points,
                                                       const double* measure, double* mean, double* volume) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= E * nc) return;
    const long long e = t / nc;
    const int c = (int)(t - e * nc);
    const bool act = !active || active[e];
    double acc = 0.0, vol = 0.0;
    if (act) {
        for (int q = 0; q < nq; ++q) {
            const double s = measure[(size_t)e * nq + q];
            vol += s;
            if (points) acc = fma(s, points[((size_t)e * nq + q) * nc + c], acc);
        }
    }
    if (mean) mean[t] = act ? acc / vol : 0.0;
    if (volume && c == 0) volume[e] = vol;
}

// nodal patch average: one thread per node over its (element, local node) entries, ascending (k_sort_n2e); an element that lists the
// node twice counts once.  A node without an active element gets zeros.
template <int NC>
__global__ void __launch_bounds__(256) k_recover_nodes(int num_nodes, int n, const unsigned* adj_off, const unsigned* adj, const unsigned char* active,
                                                       const double* mean, const double* volume, double* out) {
    const int node = blockIdx.x * 256 + threadIdx.x;
    if (node >= num_nodes) return;
    double acc[NC], vs = 0.0;
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = 0.0;
    unsigned prev = ~0u, cnt = 0;
    const unsigned k1 = adj_off[node + 1];
    for (unsigned k = adj_off[node]; k < k1; ++k) {
        const unsigned e = adj[k] / (unsigned)n;
        if (e == prev || (active && !active[e])) continue;
        prev = e;
        ++cnt;
        const double V = volume[e];
        vs += V;
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] = fma(V, mean[(size_t)e * NC + c], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) out[(size_t)node * NC + c] = cnt ? acc[c] / vs : 0.0;
}

}  // namespace fenris_hip
