// fh_dense_generalized_eigh: the small dense problem A c = w B c of the Rayleigh-Ritz step (A symmetric, B symmetric positive definite,
// p <= 96), on the host: Cholesky B = L L^T, cyclic Jacobi on L^-1 A L^-T, C = L^-T V.  No LAPACK.  Inner products of the factorisation and
// of the triangular solves are accumulated in long double.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <numeric>
#include <vector>

#include "../../include/fenris_hip.h"
#include "dense_eigh.hpp"

namespace fenris_hip_detail {

bool dense_cholesky(int p, const double* B, std::vector<double>& L) {
    L.assign((size_t)p * p, 0.0);
    for (int j = 0; j < p; ++j) {
        long double d = B[(size_t)j * p + j];
        for (int k = 0; k < j; ++k) d -= (long double)L[(size_t)j * p + k] * L[(size_t)j * p + k];
        const double dj = (double)d;
        if (!(dj > 0.0) || !std::isfinite(dj)) return false;
        const double ljj = std::sqrt(dj);
        L[(size_t)j * p + j] = ljj;
        for (int i = j + 1; i < p; ++i) {
            long double s = 0.5 * (B[(size_t)i * p + j] + B[(size_t)j * p + i]);
            for (int k = 0; k < j; ++k) s -= (long double)L[(size_t)i * p + k] * L[(size_t)j * p + k];
            L[(size_t)i * p + j] = (double)(s / ljj);
        }
    }
    return true;
}

// X <- L^-1 X (X p x q row-major, forward substitution column by column)
static void solve_lower(int p, int q, const std::vector<double>& L, double* X) {
    for (int c = 0; c < q; ++c)
        for (int i = 0; i < p; ++i) {
            long double s = X[(size_t)i * q + c];
            for (int k = 0; k < i; ++k) s -= (long double)L[(size_t)i * p + k] * X[(size_t)k * q + c];
            X[(size_t)i * q + c] = (double)(s / L[(size_t)i * p + i]);
        }
}
// X <- L^-T X (back substitution)
void dense_solve_lower_transposed(int p, int q, const std::vector<double>& L, double* X) {
    for (int c = 0; c < q; ++c)
        for (int i = p - 1; i >= 0; --i) {
            long double s = X[(size_t)i * q + c];
            for (int k = i + 1; k < p; ++k) s -= (long double)L[(size_t)k * p + i] * X[(size_t)k * q + c];
            X[(size_t)i * q + c] = (double)(s / L[(size_t)i * p + i]);
        }
}

// cyclic Jacobi (Rutishauser's rotations) on the symmetric p x p matrix H; V receives the eigenvectors by columns, the diagonal of H the
// eigenvalues.  A sweep without a rotation ends it: a pair is left alone once |h_ij| <= eps sqrt(|h_ii h_jj|) (or h_ij == 0).
static bool jacobi_eigh(int p, std::vector<double>& H, std::vector<double>& V) {
    V.assign((size_t)p * p, 0.0);
    for (int i = 0; i < p; ++i) V[(size_t)i * p + i] = 1.0;
    const double eps = 0x1p-53;
    for (int sweep = 0; sweep < 80; ++sweep) {
        bool rotated = false;
        for (int i = 0; i < p - 1; ++i)
            for (int j = i + 1; j < p; ++j) {
                const double hij = H[(size_t)i * p + j];
                if (hij == 0.0) continue;
                const double hii = H[(size_t)i * p + i], hjj = H[(size_t)j * p + j];
                if (std::fabs(hij) <= eps * std::sqrt(std::fabs(hii) * std::fabs(hjj))) continue;
                if (!std::isfinite(hij)) return false;
                rotated = true;
                const double zeta = (hjj - hii) / (2.0 * hij);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(zeta * zeta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c, tau = s / (1.0 + c);
                H[(size_t)i * p + i] = hii - t * hij;
                H[(size_t)j * p + j] = hjj + t * hij;
                H[(size_t)i * p + j] = 0.0;
                H[(size_t)j * p + i] = 0.0;
                for (int k = 0; k < p; ++k) {
                    if (k == i || k == j) continue;
                    const double hki = H[(size_t)k * p + i], hkj = H[(size_t)k * p + j];
                    const double ni = hki - s * (hkj + tau * hki), nj = hkj + s * (hki - tau * hkj);
                    H[(size_t)k * p + i] = ni;
                    H[(size_t)i * p + k] = ni;
                    H[(size_t)k * p + j] = nj;
                    H[(size_t)j * p + k] = nj;
                }
                for (int k = 0; k < p; ++k) {
                    const double vki = V[(size_t)k * p + i], vkj = V[(size_t)k * p + j];
                    V[(size_t)k * p + i] = vki - s * (vkj + tau * vki);
                    V[(size_t)k * p + j] = vkj + s * (vki - tau * vkj);
                }
            }
        if (!rotated) return true;
    }
    return false;
}

}  // namespace fenris_hip_detail

using namespace fenris_hip_detail;

extern "C" int fh_dense_generalized_eigh(uint32_t p32, const double* A, const double* B, double* w, double* C) {
    if (!A || !B || !w || !C || p32 == 0 || p32 > 96) return FH_BAD_ARGUMENT;
    const int p = (int)p32;
    for (size_t e = 0; e < (size_t)p * p; ++e)
        if (!std::isfinite(A[e]) || !std::isfinite(B[e])) return FH_EIG_BREAKDOWN;
    std::vector<double> L, H((size_t)p * p), V;
    if (!dense_cholesky(p, B, L)) return FH_EIG_BREAKDOWN;
    for (int i = 0; i < p; ++i)
        for (int j = 0; j < p; ++j) H[(size_t)i * p + j] = 0.5 * (A[(size_t)i * p + j] + A[(size_t)j * p + i]);
    solve_lower(p, p, L, H.data());                       // L^-1 A
    for (int i = 0; i < p; ++i)
        for (int j = i + 1; j < p; ++j) std::swap(H[(size_t)i * p + j], H[(size_t)j * p + i]);
    solve_lower(p, p, L, H.data());                       // L^-1 (L^-1 A)^T = L^-1 A L^-T
    for (int i = 0; i < p; ++i)
        for (int j = i + 1; j < p; ++j) {
            const double h = 0.5 * (H[(size_t)i * p + j] + H[(size_t)j * p + i]);
            H[(size_t)i * p + j] = h;
            H[(size_t)j * p + i] = h;
        }
    if (!jacobi_eigh(p, H, V)) return FH_EIG_BREAKDOWN;
    std::vector<int> order(p);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return H[(size_t)a * p + a] < H[(size_t)b * p + b]; });
    for (int j = 0; j < p; ++j) {
        w[j] = H[(size_t)order[j] * p + order[j]];
        for (int i = 0; i < p; ++i) C[(size_t)i * p + j] = V[(size_t)i * p + order[j]];
    }
    dense_solve_lower_transposed(p, p, L, C);             // C = L^-T V
    return FH_OK;
}
