// C++ host through the C ABI, no Python: a bimetal strip bends when it is heated from one end.
//   context 1: transient heat conduction (FH_LAPLACE, the theta method of fh_first_order_create) on a strip L x 1 x 1 of two Hex8 layers,
//              the end x = 0 held at T_hot above the reference temperature, everything else insulated -> nodal temperatures T
//   context 2: linear elasticity on the same mesh, the layers with different expansion coefficients;
//              fh_set_thermal_expansion(T, alpha) turns T into one stress-free stretch per element, fh_newton_solve finds the bent strip
//              (the end x = 0 clamped).  The two steps are staggered: heat, then stress.
// Prints the tip deflection across the layers and the one Timoshenko's bimetal formula gives for a uniform temperature rise of the same mean.
// Build:  make -C examples    Run: ./examples/bimetal_strip3d [cells_per_unit]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/fenris_hip.h"

#define CHECK(ctx, call)                                                                       \
    do {                                                                                       \
        int rc_ = (call);                                                                      \
        if (rc_ != FH_OK) {                                                                    \
            std::fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, fh_last_error(ctx));      \
            return 1;                                                                          \
        }                                                                                      \
    } while (0)

int main(int argc, char** argv) {
    const uint64_t cpu = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 2;
    const double L = 8.0, T_hot = 80.0, T_ref = 0.0, alpha_lo = 1.2e-5, alpha_hi = 2.3e-5;
    uint64_t nv = 0, nc = 0;
    fh_hex_mesh(1.0, (uint64_t)L, 1, 1, cpu, nullptr, nullptr, &nv, &nc);
    std::vector<double> X(3 * nv);
    std::vector<uint64_t> conn(8 * nc);
    fh_hex_mesh(1.0, (uint64_t)L, 1, 1, cpu, X.data(), conn.data(), &nv, &nc);
    std::vector<double> w(8), xi(24);
    fh_hexahedron_gauss(2, w.data(), xi.data());
    std::vector<uint64_t> hot_end;
    for (uint64_t i = 0; i < nv; ++i)
        if (X[3 * i] < 1e-12) hot_end.push_back(i);

    // ---- heat: rho c dT/dt + r(T) = 0 with the conductivity folded into the time scale (diffusivity 1), backward-weighted theta method
    fh_ctx* heat = fh_create(0);
    fh_ctx* solid = fh_create(0);
    if (!heat || !solid) { std::fprintf(stderr, "no HIP device\n"); return 2; }
    CHECK(heat, fh_set_mesh(heat, FH_HEX8, X.data(), nv, conn.data(), nc));
    CHECK(heat, fh_set_operator(heat, FH_LAPLACE));
    CHECK(heat, fh_set_quadrature_uniform(heat, w.data(), xi.data(), 8, nullptr));
    CHECK(heat, fh_set_u(heat, nullptr));
    const double capacity = 1.0;
    CHECK(heat, fh_set_mass_density(heat, &capacity, 1));
    CHECK(heat, fh_set_operator_dirichlet_nodes(heat, hot_end.data(), hot_end.size()));
    fh_first_order_settings fs{};
    fs.scheme = FH_FO_THETA;
    fs.dt = 0.5;
    fs.theta = 1.0;
    fs.newton_tolerance = 1e-9;
    fs.newton_max_iterations = 20;
    fs.line_search = FH_NEWTON_BACKTRACKING;
    fs.preconditioner = FH_PRECOND_JACOBI;
    fs.linear_rel_tol = 1e-10;
    fs.linear_max_iter = 0;
    fh_dynamics* stepper = nullptr;
    CHECK(heat, fh_first_order_create(heat, &fs, &stepper));
    std::vector<double> T(nv, T_ref);
    for (uint64_t i : hot_end) T[i] = T_hot;   // (the Dirichlet values are held where the state puts them)
    CHECK(heat, fh_dynamics_set_state(stepper, T.data(), nullptr));
    double record[4];
    uint64_t done = 0, stats[5];
    CHECK(heat, fh_dynamics_step(stepper, 16, 0, record, &done, stats));
    double time = 0.0;
    uint64_t step = 0;
    CHECK(heat, fh_dynamics_state(stepper, T.data(), nullptr, nullptr, &time, &step));
    fh_dynamics_destroy(stepper);

    // ---- stress: the two layers expand differently under that temperature
    double mu, lambda;
    fh_lame_from_young_poisson(1e7, 0.3, &mu, &lambda);
    std::vector<double> lame(16);
    for (int q = 0; q < 8; ++q) { lame[2 * q] = mu; lame[2 * q + 1] = lambda; }
    CHECK(solid, fh_set_mesh(solid, FH_HEX8, X.data(), nv, conn.data(), nc));
    CHECK(solid, fh_set_operator(solid, FH_LINEAR_ELASTIC));
    CHECK(solid, fh_set_quadrature_uniform(solid, w.data(), xi.data(), 8, lame.data()));
    CHECK(solid, fh_set_u(solid, nullptr));
    CHECK(solid, fh_set_operator_dirichlet_nodes(solid, hot_end.data(), hot_end.size()));
    std::vector<double> alpha(nc);
    for (uint64_t e = 0; e < nc; ++e) {
        double zc = 0.0;
        for (int a = 0; a < 8; ++a) zc += X[3 * conn[8 * e + a] + 2] / 8.0;
        alpha[e] = zc < 0.5 ? alpha_lo : alpha_hi;
    }
    CHECK(solid, fh_set_thermal_expansion(solid, T.data(), alpha.data(), nc, T_ref));
    std::vector<double> theta(nc), f_th(3 * nv), u(3 * nv, 0.0);
    CHECK(solid, fh_element_expansion(solid, theta.data()));
    CHECK(solid, fh_thermal_load(solid, f_th.data()));
    double fn = 0.0;
    for (double v : f_th) fn += v * v;
    uint64_t nstats[4];
    double norms[3];
    CHECK(solid, fh_newton_solve(solid, 0.0, 1.0, nullptr, nullptr, u.data(), 1e-8 * std::sqrt(fn), 20, FH_NEWTON_BACKTRACKING, FH_PRECOND_JACOBI, 1e-10,
                                 0, nstats, norms));
    double tip = 0.0, T_mean = 0.0, th_max = 0.0;
    uint64_t ntip = 0;
    for (uint64_t i = 0; i < nv; ++i) {
        T_mean += T[i] / (double)nv;
        if (X[3 * i] > L - 1e-12) { tip += u[3 * i + 2]; ++ntip; }
    }
    tip /= (double)ntip;
    for (double t : theta) th_max = std::fmax(th_max, t);
    // Timoshenko (1925), equal moduli and layer thicknesses h/2: curvature = 3 (alpha_hi - alpha_lo) dT / (2 h), tip = curvature L^2 / 2
    const double timoshenko = -1.5 * (alpha_hi - alpha_lo) * (T_mean - T_ref) * L * L / 2.0;
    std::printf("bimetal strip %ux1x1, %llu Hex8: heat %llu steps to t = %.1f (mean T %.2f, hot end %.0f), largest stretch %.6f, Newton %llu iteration(s), "
                "tip deflection %.6e (uniform-temperature bimetal formula at the mean T: %.3e)\n",
                (unsigned)L, (unsigned long long)nc, (unsigned long long)step, time, T_mean, T_hot, th_max, (unsigned long long)nstats[0], tip, timoshenko);
    fh_destroy(heat);
    fh_destroy(solid);
    // the layer that expands more lies on top: the strip bends down, by the formula's order of magnitude
    const bool ok = done == 16 && tip < 0.0 && tip / timoshenko > 0.2 && tip / timoshenko < 5.0;
    return ok ? 0 : 3;
}
