// host pieces of the dense Rayleigh-Ritz step (dense_eigh.cpp) shared with the eigensolver (engine_eigs.hip); matrices are row-major
#pragma once
#include <vector>

namespace fenris_hip_detail {
// B = L L^T (the lower triangle of the symmetrised B is read); false: a pivot is not positive (or not finite)
bool dense_cholesky(int p, const double* B, std::vector<double>& L);
// X <- L^-T X, X p x q
void dense_solve_lower_transposed(int p, int q, const std::vector<double>& L, double* X);
}  // namespace fenris_hip_detail
