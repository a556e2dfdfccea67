// C++ host, no Python: a Stable Neo-Hookean block thrown at a rigid floor.
//   unit cube of Hex8, FH_STABLE_NEO_HOOKEAN (the law that stays finite through inverted elements), density 1, initial velocity
//   (0, 0, -v0), no Dirichlet node and no load: the floor is the half-space z >= -gap of fh_set_obstacles, a penalty obstacle.
//   Central differences (fh_dynamics_step) at a quarter of the critical step of the block pressed into the floor
//   (fh_dynamics_stable_dt sees the obstacle).  Every record prints the kinetic energy, the stored energy -- elastic plus contact, the
//   column the obstacles add to -- their sum, and the lowest gap min_i phi(x_i) of fh_contact_gap_dev: the block falls, penetrates the
//   floor by a little, and comes back up with its energy kept.  With the optional pair of Rayleigh coefficients (fh_dynamics_set_damping:
//   C = eta_mass M + eta_stiffness T(u)) the block loses energy on the way and can come to rest; the critical step then is the damped one.
//   A second scene, with two more arguments: the floor gets a Coulomb coefficient (fh_set_friction, slip velocity 0.05 through
//   fh_dynamics_set_slip_velocity) and the block, resting on the floor under a weight spread evenly over its nodes (g = 10), is sent
//   sideways at v_x.  The records gain the distance its centre has slid.  A rigid block would stop after v_x^2 / (2 mu g); this soft one
//   rocks on its leading edge and stops sooner (0.067 against 0.1 with mu = 0.5, v_x = 1 on 4^3 cells), where the frictionless block of
//   the first scene would slide for ever.
// Build:  make -C examples    Run: ./examples/dropped_block3d [cells_per_unit = 4 [steps = 400 [eta_mass eta_stiffness [mu v_x]]]]
#include <hip/hip_runtime.h>

#include <algorithm>
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
#define HIP(call)                                                                              \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            std::fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_));                    \
            return 1;                                                                          \
        }                                                                                      \
    } while (0)

int main(int argc, char** argv) {
    const uint64_t cpu = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 4;
    const uint64_t steps = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 400;
    const bool damped = argc > 4;
    const double eta_mass = damped ? std::strtod(argv[3], nullptr) : 0.0, eta_stiffness = damped ? std::strtod(argv[4], nullptr) : 0.0;
    const bool sliding = argc > 6;
    const double mu_floor = sliding ? std::strtod(argv[5], nullptr) : 0.0, vx = sliding ? std::strtod(argv[6], nullptr) : 0.0, g_acc = 10.0;
    const double E = 1e3, nu = 0.3, rho = 1.0, v0 = sliding ? 0.0 : 1.0, gap = 0.02, k_floor = 2e3;
    uint64_t nv = 0, nc = 0;
    fh_hex_mesh(1.0, 1, 1, 1, cpu, nullptr, nullptr, &nv, &nc);
    std::vector<double> vertices(3 * nv);
    std::vector<uint64_t> connectivity(8 * nc);
    fh_hex_mesh(1.0, 1, 1, 1, cpu, vertices.data(), connectivity.data(), &nv, &nc);
    std::vector<double> w(8), xi(24);
    fh_hexahedron_gauss(2, w.data(), xi.data());
    double mu, lambda;
    fh_lame_from_young_poisson(E, nu, &mu, &lambda);
    fh_stable_neo_hookean_parameters(3, mu, lambda, &mu, &lambda);
    std::vector<double> lame(16);
    for (int q = 0; q < 8; ++q) { lame[2 * q] = mu; lame[2 * q + 1] = lambda; }

    fh_ctx* ctx = fh_create(0);
    if (!ctx) { std::fprintf(stderr, "no HIP device\n"); return 2; }
    CHECK(ctx, fh_set_mesh(ctx, FH_HEX8, vertices.data(), nv, connectivity.data(), nc));
    CHECK(ctx, fh_set_operator(ctx, FH_STABLE_NEO_HOOKEAN));
    CHECK(ctx, fh_set_quadrature_uniform(ctx, w.data(), xi.data(), 8, lame.data()));
    CHECK(ctx, fh_set_mass_density(ctx, &rho, 1));
    fh_obstacle floor{};
    floor.kind = FH_OBSTACLE_HALF_SPACE;
    floor.stiffness = k_floor * 4.0 / double(cpu * cpu);   // per node: the floor's stiffness per area stays as the mesh is refined
    floor.point[2] = -gap;
    floor.normal[2] = 1.0;
    CHECK(ctx, fh_set_obstacles(ctx, &floor, 1, nullptr));
    if (sliding) CHECK(ctx, fh_set_friction(ctx, &mu_floor, 1, 1e-3));   // (the integrator replaces the slip length by slip velocity x dt)

    const size_t n = 3 * nv;
    std::vector<double> u(n, 0.0), v(n, 0.0);
    fh_dynamics_settings s{};
    s.scheme = FH_DYN_CENTRAL_DIFFERENCE;
    s.dt = 1.0;
    fh_dynamics* probe = nullptr;
    CHECK(ctx, fh_dynamics_create(ctx, &s, &probe));
    for (size_t i = 0; i < nv; ++i) u[3 * i + 2] = -2.0 * gap;   // the bottom face inside the floor: the stiffest state of the run
    CHECK(ctx, fh_dynamics_set_state(probe, u.data(), nullptr));
    if (damped) CHECK(ctx, fh_dynamics_set_damping(probe, eta_mass, eta_stiffness));
    double omega = 0.0, dt_crit = 0.0;
    CHECK(ctx, fh_dynamics_stable_dt(probe, 40, &omega, &dt_crit));
    fh_dynamics_destroy(probe);
    s.dt = 0.25 * dt_crit;

    fh_dynamics* dyn = nullptr;
    CHECK(ctx, fh_dynamics_create(ctx, &s, &dyn));
    if (damped) CHECK(ctx, fh_dynamics_set_damping(dyn, eta_mass, eta_stiffness));
    std::fill(u.begin(), u.end(), 0.0);
    for (size_t i = 0; i < nv; ++i) v[3 * i + 2] = -v0;
    if (sliding) {   // resting on the floor, each node carrying its share of the weight, and moving sideways
        CHECK(ctx, fh_dynamics_set_slip_velocity(dyn, 0.05));
        const double share = rho * g_acc / double(nv);
        std::vector<double> weight(n, 0.0);
        for (size_t i = 0; i < nv; ++i) {
            weight[3 * i + 2] = -share;
            u[3 * i + 2] = -gap - share * double(nv) / (floor.stiffness * double((cpu + 1) * (cpu + 1)));
            v[3 * i] = vx;
        }
        CHECK(ctx, fh_dynamics_set_load(dyn, weight.data(), nullptr, 0));
    }
    CHECK(ctx, fh_dynamics_set_state(dyn, u.data(), v.data()));
    double* gap_dev = nullptr;
    HIP(hipMalloc(&gap_dev, sizeof(double) * nv));
    std::vector<double> gaps(nv);
    const uint64_t every = std::max<uint64_t>(1, steps / 10);
    std::printf("dropped_block3d: %llu Hex8, dt = %.4e (omega_max = %.1f with the floor), floor z >= %.3f, k = %.1f per node\n",
                (unsigned long long)nc, s.dt, omega, -gap, floor.stiffness);
    if (damped) std::printf("dropped_block3d: Rayleigh damping eta_mass = %g, eta_stiffness = %g\n", eta_mass, eta_stiffness);
    std::printf("%10s %12s %12s %12s %12s\n", "time", "kinetic", "stored", "total", "lowest gap");
    double first_total = 0.0, last_total = 0.0, lowest = 1e300;
    for (uint64_t done = 0; done < steps; done += every) {
        double row[4];
        uint64_t took = 0, stats[5];
        CHECK(ctx, fh_dynamics_step(dyn, std::min(every, steps - done), 0, row, &took, stats));
        CHECK(ctx, fh_contact_gap_dev(ctx, gap_dev));
        HIP(hipMemcpy(gaps.data(), gap_dev, sizeof(double) * nv, hipMemcpyDeviceToHost));
        const double g = *std::min_element(gaps.begin(), gaps.end());
        lowest = std::min(lowest, g);
        last_total = row[0] + row[1];
        if (done == 0) first_total = last_total;
        std::printf("%10.4f %12.6f %12.6f %12.6f %12.5f", row[3], row[0], row[1], last_total, g);
        if (sliding) {
            CHECK(ctx, fh_dynamics_state(dyn, u.data(), nullptr, nullptr, nullptr, nullptr));
            double ux = 0.0;
            for (size_t i = 0; i < nv; ++i) ux += u[3 * i] / double(nv);
            std::printf("   slid %.5f", ux);
        }
        std::printf("\n");
    }
    CHECK(ctx, fh_dynamics_state(dyn, u.data(), v.data(), nullptr, nullptr, nullptr));
    double vz = 0.0;
    for (size_t i = 0; i < nv; ++i) vz += v[3 * i + 2] / double(nv);
    std::printf("dropped_block3d: mean v_z %+.3f (thrown at %+.3f), deepest gap %.4f, total energy %.5f -> %.5f, kernel %s\n", vz, -v0, lowest,
                first_total, last_total, fh_last_kernel_name(ctx));
    if (sliding) {
        double ux = 0.0, vxm = 0.0;
        for (size_t i = 0; i < nv; ++i) { ux += u[3 * i] / double(nv); vxm += v[3 * i] / double(nv); }
        std::printf("dropped_block3d: mu = %g, sent off at v_x = %g: the centre has slid %.5f and moves at %+.5f (v_x^2 / (2 mu g) = %.5f)\n", mu_floor, vx,
                    ux, vxm, mu_floor > 0.0 ? vx * vx / (2.0 * mu_floor * g_acc) : INFINITY);
    }
    HIP(hipFree(gap_dev));
    fh_dynamics_destroy(dyn);
    fh_destroy(ctx);
    return 0;
}
