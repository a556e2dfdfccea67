// The material laws of the elliptic operators, written once: stress and energy density of a quadrature point (material_point), the
// tangent of the stress (tangent_lin / tangent_apply) and the point's Lame parameters (point_params).  Every element kernel that needs a
// stress calls these: the register-resident element pass and the tiles (element_pass.hpp, vector_tiles.hip), the LDS-staged vector and
// scalar kernels (prologue() of assemble_kernels.hpp), the matrix-free kernels of solver_kernels.hpp and recovery (recover_kernels.hpp).
// (The coefficients of the assembled matrices -- the matrix branch of prologue(), hex27_blocks.hpp -- are not stresses and stay there.)
// Only __device__ __forceinline__ functions: safe to include from several translation units.
#pragma once
#include <hip/hip_runtime.h>

#include "device_common.hpp"
#include "small_ops.hpp"

namespace fenris_hip {

enum { EP_VECTOR = 0, EP_SCALAR = 1 };

// F = I + (grad u)^T from gu[i][k] = d u_k / d X_i  (fenris-solid/src/lib.rs:20-29)
template <int D, int S>
__device__ __forceinline__ void deformation_gradient(const double (&gu)[D][S], double (&F)[D][D]) {
    static_assert(S == D, "a deformation gradient needs a vector field");
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) F[i][j] = (i == j ? 1.0 : 0.0) + gu[j][i];
}
// Green strain E = (F^T F - I) / 2  (green_strain_tensor)
template <int D>
__device__ __forceinline__ void green_strain(const double (&F)[D][D], double (&E)[D][D]) {
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) {
            double t = 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) t = fma(F[k][i], F[k][j], t);
            E[i][j] = (t - (i == j ? 1.0 : 0.0)) * 0.5;
        }
}

// gamma = det(I + U) - 1 expanded in U, so that it keeps its relative precision where det F is close to 1 (logdet.rs:17-86)
template <int D>
__device__ __forceinline__ double det_minus_one(const double (&U)[D][D]) {
    if constexpr (D == 2) {
        return U[0][0] * U[1][1] + U[0][0] + U[1][1] - U[0][1] * U[1][0];
    } else {
        const double u11 = U[0][0], u22 = U[1][1], u33 = U[2][2];
        const double aa = 1.0 + u11, e2 = 1.0 + u22, i2 = 1.0 + u33;
        const double b = U[0][1], c = U[0][2], d2 = U[1][0], f = U[1][2], g = U[2][0], h = U[2][1];
        return u11 * u22 * u33 + u11 * u22 + u11 * u33 + u22 * u33 + u11 + u22 + u33 + b * f * g + c * d2 * h -
               c * e2 * g - b * d2 * i2 - aa * f * h;
    }
}
// cof F = dJ/dF, and its derivative along H written out from the entries (linear in H): the H x F cross terms in 3-D, the 2 x 2 swap in 2-D
template <int D>
__device__ __forceinline__ void cofactor(const double (&F)[D][D], double (&C)[D][D]) {
    if constexpr (D == 2) {
        C[0][0] = F[1][1]; C[0][1] = -F[1][0];
        C[1][0] = -F[0][1]; C[1][1] = F[0][0];
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
                C[i][j] = F[i1][j1] * F[i2][j2] - F[i1][j2] * F[i2][j1];
            }
    }
}
template <int D>
__device__ __forceinline__ void cofactor_lin(const double (&F)[D][D], const double (&H)[D][D], double (&dC)[D][D]) {
    if constexpr (D == 2) {
        dC[0][0] = H[1][1]; dC[0][1] = -H[1][0];
        dC[1][0] = -H[0][1]; dC[1][1] = H[0][0];
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
                dC[i][j] = fma(H[i1][j1], F[i2][j2], F[i1][j1] * H[i2][j2]) - fma(H[i1][j2], F[i2][j1], F[i1][j2] * H[i2][j1]);
            }
    }
}
// What Stable Neo-Hookean takes from grad u at a point (fenris_hip.h, FH_STABLE_NEO_HOOKEAN): F, cof F, c = F:F - d and gamma = det F - 1.
// Polynomial in U; nothing here or in what follows branches on det F.
template <int D, int S>
__device__ __forceinline__ void snh_kinematics(const double (&gu)[D][S], double (&F)[D][D], double (&C)[D][D], double& c, double& gamma) {
    static_assert(S == D, "a deformation gradient needs a vector field");
    double U[D][D];
    double trU = 0.0, nn = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int j = 0; j < D; ++j) {
            U[i][j] = gu[j][i];
            F[i][j] = (i == j ? 1.0 : 0.0) + U[i][j];
            nn = fma(U[i][j], U[i][j], nn);
        }
#pragma unroll
    for (int i = 0; i < D; ++i) trU += U[i][i];
    c = fma(2.0, trU, nn);
    gamma = det_minus_one<D>(U);
    cofactor<D>(F, C);
}
// its three coefficients: a0 = mu (1 - 1/m) written as mu (d + c)/m, a1 = 2 mu/m^2 and b = lambda gamma - k with m = d + 1 + c >= 1 and
// k = mu d/(d + 1).  At F = I (c = 0, gamma = 0) a0 and k are the same product, so P(I) = a0 I - k I = 0 exactly.
template <int D>
__device__ __forceinline__ void snh_coefficients(double mu, double lambda, double c, double gamma, double& a0, double& a1, double& b) {
    const double m = (double)(D + 1) + c;
    a0 = mu * (((double)D + c) / m);
    a1 = 2.0 * mu / (m * m);
    b = fma(lambda, gamma, -(mu * ((double)D / (double)(D + 1))));
}

// stress P (s x d) and energy density psi of one quadrature point from grad u (d x s):
// laplace.rs:26-73; fenris-solid/src/materials.rs:71-123 (LinearElastic), 236-353 (NeoHookean, J <= 0 => NaN block / inf),
// 392-469 (StVK); Stable Neo-Hookean: fenris_hip.h, FH_STABLE_NEO_HOOKEAN (finite for every F).
template <int OP, int D, int S, int WHAT>
__device__ __forceinline__ void material_point(const double (&gu)[D][S], double mu, double lambda, double (&P)[S][D], double& psi) {
    psi = 0.0;
    if constexpr (OP == FH_LAPLACE) {
#pragma unroll
        for (int k = 0; k < D; ++k) { P[0][k] = gu[k][0]; psi = fma(gu[k][0], gu[k][0], psi); }
        psi *= 0.5;
    } else if constexpr (OP == FH_STABLE_NEO_HOOKEAN) {
        double F[D][D], C[D][D];
        double c, gamma;
        snh_kinematics<D, S>(gu, F, C, c, gamma);
        double a0, a1, b;
        snh_coefficients<D>(mu, lambda, c, gamma, a0, a1, b);
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) P[i][j] = fma(a0, F[i][j], b * C[i][j]);
        if constexpr (WHAT == EP_SCALAR)
            psi = (0.5 * mu) * (c - log1p(c / (double)(D + 1))) + (0.5 * lambda) * (gamma * gamma) - mu * ((double)D / (double)(D + 1)) * gamma;
    } else {
        double F[D][D];
        deformation_gradient<D, S>(gu, F);
        if constexpr (OP == FH_LINEAR_ELASTIC) {
            double eps[D][D];
            double tr = 0.0, ee = 0.0;
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    eps[i][j] = (F[j][i] + F[i][j]) * 0.5 - (i == j ? 1.0 : 0.0);
                    ee = fma(eps[i][j], eps[i][j], ee);
                }
#pragma unroll
            for (int i = 0; i < D; ++i) tr += eps[i][i];
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int j = 0; j < D; ++j) P[i][j] = eps[i][j] * 2.0 * mu + (i == j ? lambda * tr : 0.0);
            psi = mu * ee + 0.5 * lambda * (tr * tr);
        } else if constexpr (OP == FH_NEO_HOOKEAN) {
            const double Jd = det_small<D>(F);
            if (Jd <= 0.0) {
#pragma unroll
                for (int i = 0; i < D; ++i)
#pragma unroll
                    for (int j = 0; j < D; ++j) P[i][j] = __builtin_nan("");
            } else {
                double Fi[D][D];
                inv_small(F, Jd, Fi);
                const double c = -mu + lambda * log(Jd);
#pragma unroll
                for (int i = 0; i < D; ++i)
#pragma unroll
                    for (int j = 0; j < D; ++j) P[i][j] = Fi[j][i] * c + F[i][j] * mu;
            }
            if constexpr (WHAT == EP_SCALAR) {
                // materials.rs:249-262 with log_det_F of du_dX = (grad u)^T (logdet.rs:17-86)
                double U[D][D];
#pragma unroll
                for (int i = 0; i < D; ++i)
#pragma unroll
                    for (int j = 0; j < D; ++j) U[i][j] = gu[j][i];
                const double gamma = det_minus_one<D>(U);
                if (gamma > -1.0) {
                    const double logJ = log1p(gamma);
                    double trU = 0.0, nn = 0.0;
#pragma unroll
                    for (int i = 0; i < D; ++i) {
                        trU += U[i][i];
#pragma unroll
                        for (int j = 0; j < D; ++j) nn = fma(U[i][j], U[i][j], nn);
                    }
                    psi = mu * (trU + 0.5 * nn) - mu * logJ + (0.5 * lambda) * (logJ * logJ);
                } else {
                    psi = __builtin_inf();
                }
            }
        } else {  // StVK: P = F E 2 mu + F lambda tr E ; psi = mu E:E + lambda/2 tr^2
            double Eg[D][D];
            double trE = 0.0, ee = 0.0;
            green_strain<D>(F, Eg);
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int j = 0; j < D; ++j) ee = fma(Eg[i][j], Eg[i][j], ee);
#pragma unroll
            for (int i = 0; i < D; ++i) trE += Eg[i][i];
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int j = 0; j < D; ++j) {
                    double t = 0.0;
#pragma unroll
                    for (int k = 0; k < D; ++k) t = fma(F[i][k], Eg[k][j], t);
                    P[i][j] = t * 2.0 * mu + F[i][j] * lambda * trE;
                }
            psi = mu * ee + 0.5 * lambda * (trE * trE);
        }
    }
}

// ---- tangent of the stress: T(u) = dr/du at the context's u is applied without the matrix (engine_vector.hip).  Per point the element vector
// of the operand x is  y_a += w |det J| dP(F)[H] g_a  with F = I + grad u^T, H = grad x^T (x enters linearly: I + grad x is never formed):
//   Laplace        h
//   LinearElastic  mu (H + H^T) + lambda tr(H) I
//   NeoHookean     mu H + lambda tr(F^-1 H) F^-T + (mu - lambda ln J) F^-T H^T F^-T        (J <= 0: NaN, materials.rs:297-300)
//   StVK           H S + F (lambda tr(dE) I + 2 mu dE),  S = lambda tr(E) I + 2 mu E,  dE = sym(F^T H)
//   Stable NH      mu (1 - 1/m) H + 2 mu/m^2 (F:H) F + lambda (cof F:H) cof F + (lambda gamma - k) dcof(F)[H],  m = d + 1 + F:F - d
// which is  sum_b C(F; g_a, g_b) x_b  with C the stress contraction the assembled K(u) is made of (materials.rs:287-315 and 417-439).
// TangentLin holds what depends on u alone (formed once per point); tangent_apply is linear in grad x.
template <int OP, int D>
struct TangentLin {
    double mu, lambda, beta;   // NeoHookean: beta = mu - lambda ln J
    double F[D][D];            // NeoHookean: F^-1; StVK: F
    double Sg[D][D];           // StVK: the second Piola-Kirchhoff stress S
};
template <int D>
struct TangentLin<FH_STABLE_NEO_HOOKEAN, D> {
    double a0, a1, lambda, b;   // mu (1 - 1/m), 2 mu/m^2, lambda, lambda gamma - k
    double F[D][D], C[D][D];    // F and cof F
};
template <int OP, int D, int S>
__device__ __forceinline__ void tangent_lin(const double (&gu)[D][S], double mu, double lambda, TangentLin<OP, D>& L) {
    if constexpr (OP == FH_STABLE_NEO_HOOKEAN) {
        double c, gamma;
        snh_kinematics<D, S>(gu, L.F, L.C, c, gamma);
        snh_coefficients<D>(mu, lambda, c, gamma, L.a0, L.a1, L.b);
        L.lambda = lambda;
        return;
    } else {
        L.mu = mu;
        L.lambda = lambda;
    }
    if constexpr (OP == FH_NEO_HOOKEAN || OP == FH_STVK) {
        double F[D][D];
        deformation_gradient<D, S>(gu, F);
        if constexpr (OP == FH_NEO_HOOKEAN) {
            const double Jd = det_small<D>(F);
            if (Jd <= 0.0) {
#pragma unroll
                for (int i = 0; i < D; ++i)
#pragma unroll
                    for (int j = 0; j < D; ++j) L.F[i][j] = __builtin_nan("");
                L.beta = __builtin_nan("");
            } else {
                inv_small(F, Jd, L.F);
                L.beta = mu - lambda * log(Jd);
            }
        } else {
            double trE = 0.0;
            green_strain<D>(F, L.Sg);   // E, overwritten by S below
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int j = 0; j < D; ++j) L.F[i][j] = F[i][j];
#pragma unroll
            for (int i = 0; i < D; ++i) trE += L.Sg[i][i];
#pragma unroll
            for (int i = 0; i < D; ++i)
#pragma unroll
                for (int j = 0; j < D; ++j) L.Sg[i][j] = L.Sg[i][j] * 2.0 * mu + (i == j ? lambda * trE : 0.0);
        }
    }
}
// dP (s x d) from gx = grad x (d x s, gx[i][k] = d x_k / d X_i)
template <int OP, int D, int S>
__device__ __forceinline__ void tangent_apply(const TangentLin<OP, D>& L, const double (&gx)[D][S], double (&dP)[S][D]) {
    if constexpr (OP == FH_LAPLACE) {
#pragma unroll
        for (int r = 0; r < D; ++r) dP[0][r] = gx[r][0];
    } else if constexpr (OP == FH_LINEAR_ELASTIC) {
        double tr = 0.0;
#pragma unroll
        for (int i = 0; i < D; ++i) tr += gx[i][i];
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) dP[i][j] = L.mu * (gx[j][i] + gx[i][j]) + (i == j ? L.lambda * tr : 0.0);
    } else if constexpr (OP == FH_NEO_HOOKEAN) {
        double A[D][D], tr = 0.0;   // A = F^-1 H
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) {
                double t = 0.0;
#pragma unroll
                for (int k = 0; k < D; ++k) t = fma(L.F[i][k], gx[j][k], t);
                A[i][j] = t;
            }
#pragma unroll
        for (int i = 0; i < D; ++i) tr += A[i][i];
        const double lt = L.lambda * tr;
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) {
                double b = 0.0;   // (F^-1 H F^-1)[j][i]
#pragma unroll
                for (int k = 0; k < D; ++k) b = fma(A[j][k], L.F[k][i], b);
                dP[i][j] = fma(L.beta, b, fma(lt, L.F[j][i], L.mu * gx[j][i]));
            }
    } else if constexpr (OP == FH_STABLE_NEO_HOOKEAN) {
        double H[D][D], dC[D][D];
        double fh = 0.0, ch = 0.0;   // F:H, cof F:H
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) {
                H[i][j] = gx[j][i];
                fh = fma(L.F[i][j], H[i][j], fh);
                ch = fma(L.C[i][j], H[i][j], ch);
            }
        cofactor_lin<D>(L.F, H, dC);
        const double f1 = L.a1 * fh, c1 = L.lambda * ch;
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) dP[i][j] = fma(L.a0, H[i][j], fma(f1, L.F[i][j], fma(c1, L.C[i][j], L.b * dC[i][j])));
    } else {   // StVK
        double C[D][D];   // F^T H
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) {
                double t = 0.0;
#pragma unroll
                for (int k = 0; k < D; ++k) t = fma(L.F[k][i], gx[j][k], t);
                C[i][j] = t;
            }
        double tr = 0.0;
#pragma unroll
        for (int i = 0; i < D; ++i) tr += C[i][i];
        double T[D][D];   // lambda tr(dE) I + 2 mu dE
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) T[i][j] = L.mu * (C[i][j] + C[j][i]) + (i == j ? L.lambda * tr : 0.0);
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int j = 0; j < D; ++j) {
                double t = 0.0;
#pragma unroll
                for (int k = 0; k < D; ++k) t = fma(gx[k][i], L.Sg[k][j], fma(L.F[i][k], T[k][j], t));
                dP[i][j] = t;
            }
    }
}
// ---- per-element expansion (fh_set_element_expansion): theta > 0 is the stress-free isotropic stretch of the element, 1 = none.
//   LinearElastic (additive):      gu_e = gu - (theta - 1) I,            P = P_0(gu_e),              psi = psi_0(gu_e),          dP = dP_0
//   hyperelastic (F = F_e theta):  gu_e = (gu - (theta - 1) I) / theta,  P = theta^(d-1) P_0(gu_e),  psi = theta^d psi_0(gu_e),  dP[H] = theta^(d-2) dP_0(gu_e)[H]
// The laws above stay as they are: a kernel changes their argument and scales their result.  Within an element (theta - 1) I is the gradient of
// (theta - 1)(X - X_0), so the register-resident bodies take the law through their nodal values, U'_n = (U_n - (theta - 1)(X_n - X_0)) / theta
// (stretch_nodes: relative to the element's node 0, so that coordinates far from the origin do not cancel; U' of a trilinear U is trilinear,
// the Hex8 moment form stays exact); the kernels that hold grad u at a point take it there (stretch_strain).  Powers by multiplication.
// theta == 1 changes no bit of either form: the subtrahend is a zero, the factors are 1.
template <int OP, int D>
struct Stretch {
    static_assert(OP == FH_LINEAR_ELASTIC || OP == FH_NEO_HOOKEAN || OP == FH_STVK || OP == FH_STABLE_NEO_HOOKEAN, "the expansion strains an elastic operator");
    static constexpr bool additive = OP == FH_LINEAR_ELASTIC;
    double t1;    // theta - 1
    double inv;   // 1 / theta; additive: 1
    double sT;    // theta^(d-2), the factor of the tangent; additive: 1
    double sP;    // theta^(d-1), of the stress
    double sPsi;  // theta^d, of the energy density
    __device__ __forceinline__ explicit Stretch(double theta) {
        t1 = theta - 1.0;
        if constexpr (additive) {
            inv = 1.0; sT = 1.0; sP = 1.0; sPsi = 1.0;
        } else {
            inv = 1.0 / theta;
            sT = D == 3 ? theta : 1.0;
            sP = sT * theta;
            sPsi = sP * theta;
        }
    }
};
// the stretch of element e from the arguments (KArgs::theta: one for the mesh or one per element)
template <int OP, int D>
__device__ __forceinline__ Stretch<OP, D> element_stretch(const KArgs& a, long long e) {
    return Stretch<OP, D>(a.theta[a.theta_per_elem ? e : 0]);
}
// grad u -> the elastic part gu_e, at a point
template <int OP, int D, int S>
__device__ __forceinline__ void stretch_strain(const Stretch<OP, D>& st, double (&gu)[D][S]) {
    static_assert(S == D, "the expansion strains a vector field");
#pragma unroll
    for (int i = 0; i < D; ++i) gu[i][i] -= st.t1;
    if constexpr (!Stretch<OP, D>::additive) {
#pragma unroll
        for (int i = 0; i < D; ++i)
#pragma unroll
            for (int k = 0; k < S; ++k) gu[i][k] *= st.inv;
    }
}
// the nodal values whose gradient is gu_e, in place: U'_n = (U_n - (theta - 1)(X_n - X_0)) / theta
template <int OP, int D, int N>
__device__ __forceinline__ void stretch_nodes(const Stretch<OP, D>& st, const double (&X)[N][D], double (&U)[N][D]) {
#pragma unroll
    for (int n = 0; n < N; ++n)
#pragma unroll
        for (int k = 0; k < D; ++k) {
            const double v = n == 0 ? U[n][k] : fma(-st.t1, X[n][k] - X[0][k], U[n][k]);
            U[n][k] = Stretch<OP, D>::additive ? v : v * st.inv;
        }
}
// f *= s over an element vector (the hyperelastic factors; the additive law has none)
template <int OP, int D, int N, int S>
__device__ __forceinline__ void stretch_scale(double s, double (&f)[N][S]) {
    if constexpr (!Stretch<OP, D>::additive) {
#pragma unroll
        for (int n = 0; n < N; ++n)
#pragma unroll
            for (int k = 0; k < S; ++k) f[n][k] *= s;
    }
}
// whether an operator has an instantiation with the expansion (FH_LAPLACE and FH_TENSOR are refused on the host)
__host__ __device__ constexpr bool op_expands(int op) {
    return op == FH_LINEAR_ELASTIC || op == FH_NEO_HOOKEAN || op == FH_STVK || op == FH_STABLE_NEO_HOOKEAN;
}

// the Lame parameters of point q: the element's own (par_e: its row of a compact table, KArgs::rparams) or the uniform table's, by scalar loads
template <int OP>
__device__ __forceinline__ void point_params(const KArgs& a, const double* par_e, int q, double& mu, double& lambda) {
    mu = 0.0;
    lambda = 0.0;
    if (OP != FH_LAPLACE) {
        if (par_e) { mu = par_e[2 * q]; lambda = par_e[2 * q + 1]; }
        else { mu = ep_const(a.qparams)[2 * q]; lambda = ep_const(a.qparams)[2 * q + 1]; }
    }
}

}  // namespace fenris_hip
