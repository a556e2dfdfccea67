// C++ host, no Python: a rigid ball pressed into a clamped block along a path, and a floor that slides away under one.
//   Scene 1.  Unit cube of Hex8, FH_LINEAR_ELASTIC, clamped on its bottom face (fh_set_operator_dirichlet_nodes).  A ball of radius 1
//   (fh_set_obstacles) rests on the middle of the top face and follows a path (fh_set_obstacle_paths): pressed in by `depth` over the
//   first third of the run, held for a third, retracted past its start over the last.  Backward Euler (fh_dynamics_step) moves the contact
//   clock itself; after every record the example prints the time, the ball's indentation (fh_obstacle_offsets) and the force the block
//   exerts on it, R_o of fh_contact_resultants: the force-indentation curve of the run.
//   Scene 2.  The same cube, free, resting 0.01 inside the floor z >= 0 with a Coulomb coefficient (fh_set_friction); the floor slides
//   along x at a constant velocity (a two-knot path) under central differences.  The friction slip is taken relative to the floor, so the
//   floor drags the block along: the records print the mean velocity of the block and the force R_z it presses on the floor with.
// Build:  make -C examples    Run: ./examples/indented_block3d [cells_per_unit = 4 [steps = 60 [depth = 0.05]]]
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

int main(int argc, char** argv) {
    const uint64_t cpu = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 4;
    const uint64_t steps = argc > 2 ? std::max<uint64_t>(6, std::strtoull(argv[2], nullptr, 10)) : 60;
    const double depth = argc > 3 ? std::strtod(argv[3], nullptr) : 0.05;
    const double E = 1e3, nu = 0.3, rho = 1.0;
    uint64_t nv = 0, nc = 0;
    fh_hex_mesh(1.0, 1, 1, 1, cpu, nullptr, nullptr, &nv, &nc);
    std::vector<double> vertices(3 * nv);
    std::vector<uint64_t> connectivity(8 * nc);
    fh_hex_mesh(1.0, 1, 1, 1, cpu, vertices.data(), connectivity.data(), &nv, &nc);
    std::vector<double> w(8), xi(24);
    fh_hexahedron_gauss(2, w.data(), xi.data());
    double mu, lambda;
    fh_lame_from_young_poisson(E, nu, &mu, &lambda);
    std::vector<double> lame(16);
    for (int q = 0; q < 8; ++q) { lame[2 * q] = mu; lame[2 * q + 1] = lambda; }
    const size_t n = 3 * nv;
    const double k_node = 2e3 * 4.0 / double(cpu * cpu);   // per node: the stiffness per area stays as the mesh is refined

    fh_ctx* ctx = fh_create(0);
    if (!ctx) { std::fprintf(stderr, "no HIP device\n"); return 2; }
    CHECK(ctx, fh_set_mesh(ctx, FH_HEX8, vertices.data(), nv, connectivity.data(), nc));
    CHECK(ctx, fh_set_operator(ctx, FH_LINEAR_ELASTIC));
    CHECK(ctx, fh_set_quadrature_uniform(ctx, w.data(), xi.data(), 8, lame.data()));
    CHECK(ctx, fh_set_mass_density(ctx, &rho, 1));

    // ---- scene 1: the indenter
    std::vector<uint64_t> bottom;
    for (uint64_t i = 0; i < nv; ++i)
        if (vertices[3 * i + 2] == 0.0) bottom.push_back(i);
    CHECK(ctx, fh_set_operator_dirichlet_nodes(ctx, bottom.data(), bottom.size()));
    fh_obstacle ball{};
    ball.kind = FH_OBSTACLE_BALL;
    ball.stiffness = k_node;
    ball.radius = 1.0;
    ball.point[0] = ball.point[1] = 0.5;
    ball.point[2] = 2.0;   // touching the top face at its middle
    CHECK(ctx, fh_set_obstacles(ctx, &ball, 1, nullptr));
    fh_dynamics_settings s{};
    s.scheme = FH_DYN_BACKWARD_EULER;
    s.dt = 0.02;
    s.newton_tolerance = 1e-10;
    s.newton_max_iterations = 40;
    s.line_search = FH_NEWTON_BACKTRACKING;
    s.preconditioner = FH_PRECOND_JACOBI;
    s.linear_rel_tol = 1e-10;
    const double T = double(steps) * s.dt;
    const uint64_t knot_begin[2] = {0, 4};
    const double knot_time[4] = {0.0, T / 3.0, 2.0 * T / 3.0, T};
    const double knot_offset[12] = {0.0, 0.0, 0.0, 0.0, 0.0, -depth, 0.0, 0.0, -depth, 0.0, 0.0, 0.5 * depth};
    CHECK(ctx, fh_set_obstacle_paths(ctx, knot_begin, knot_time, knot_offset));
    fh_dynamics* dyn = nullptr;
    CHECK(ctx, fh_dynamics_create(ctx, &s, &dyn));
    CHECK(ctx, fh_dynamics_set_state(dyn, nullptr, nullptr));
    const uint64_t every = std::max<uint64_t>(1, steps / 12);
    std::printf("indented_block3d: %llu Hex8 clamped at z = 0, a ball of radius 1 pressed in by %.3f, held, retracted; backward Euler, dt = %.3f\n",
                (unsigned long long)nc, depth, s.dt);
    std::printf("%10s %14s %14s %14s\n", "time", "indentation", "force on ball", "stored energy");
    double peak = 0.0, last = 0.0;
    for (uint64_t done = 0; done < steps; done += every) {
        double row[4], offset[3], R[3];
        uint64_t took = 0, stats[5];
        CHECK(ctx, fh_dynamics_step(dyn, std::min(every, steps - done), 0, row, &took, stats));
        CHECK(ctx, fh_obstacle_offsets(ctx, offset, nullptr));
        CHECK(ctx, fh_contact_resultants(ctx, R, nullptr));
        peak = std::max(peak, std::fabs(R[2]));
        last = std::sqrt(R[0] * R[0] + R[1] * R[1] + R[2] * R[2]);
        std::printf("%10.4f %14.5f %14.6f %14.6f\n", row[3], -offset[2], R[2], row[1]);
    }
    if (last == 0.0) std::printf("indented_block3d: peak force %.6f; retracted, the ball is clear of the block\n", peak);
    else std::printf("indented_block3d: peak force %.6f; the block still presses on the retracted ball with %.6f\n", peak, last);
    fh_dynamics_destroy(dyn);

    // ---- scene 2: the sliding floor
    CHECK(ctx, fh_set_operator_dirichlet_nodes(ctx, nullptr, 0));
    fh_obstacle floor{};
    floor.kind = FH_OBSTACLE_HALF_SPACE;
    floor.stiffness = k_node;
    floor.normal[2] = 1.0;
    CHECK(ctx, fh_set_obstacles(ctx, &floor, 1, nullptr));
    const double mu_floor = 0.5, belt = 0.2;
    CHECK(ctx, fh_set_friction(ctx, &mu_floor, 1, 1e-3));   // (the integrator replaces the slip length by slip velocity x dt)
    fh_dynamics_settings e{};
    e.scheme = FH_DYN_CENTRAL_DIFFERENCE;
    e.dt = 1.0;
    std::vector<double> u(n, 0.0), v(n, 0.0);
    for (size_t i = 0; i < nv; ++i) u[3 * i + 2] = -0.01;
    fh_dynamics* probe = nullptr;
    CHECK(ctx, fh_dynamics_create(ctx, &e, &probe));
    CHECK(ctx, fh_dynamics_set_state(probe, u.data(), nullptr));
    double omega = 0.0, dt_crit = 0.0;
    CHECK(ctx, fh_dynamics_stable_dt(probe, 40, &omega, &dt_crit));
    fh_dynamics_destroy(probe);
    e.dt = 0.25 * dt_crit;
    const uint64_t slide_steps = 20 * steps;
    const uint64_t kb[2] = {0, 2};
    const double kt[2] = {0.0, double(slide_steps) * e.dt};
    const double ko[6] = {0.0, 0.0, 0.0, belt * kt[1], 0.0, 0.0};
    CHECK(ctx, fh_set_obstacle_paths(ctx, kb, kt, ko));
    CHECK(ctx, fh_dynamics_create(ctx, &e, &dyn));
    CHECK(ctx, fh_dynamics_set_slip_velocity(dyn, 0.05));
    const double share = rho * 10.0 / double(nv);
    std::vector<double> weight(n, 0.0);
    for (size_t i = 0; i < nv; ++i) weight[3 * i + 2] = -share;
    CHECK(ctx, fh_dynamics_set_load(dyn, weight.data(), nullptr, 0));
    CHECK(ctx, fh_dynamics_set_state(dyn, u.data(), v.data()));
    std::printf("indented_block3d: the floor slides along x at %.2f with mu = %.1f under the free block; central differences, dt = %.3e\n", belt,
                mu_floor, e.dt);
    std::printf("%10s %14s %14s %14s\n", "time", "floor moved", "mean v_x", "force on floor");
    const uint64_t every2 = std::max<uint64_t>(1, slide_steps / 10);
    for (uint64_t done = 0; done < slide_steps; done += every2) {
        double row[4], offset[3], R[3];
        uint64_t took = 0, stats[5];
        CHECK(ctx, fh_dynamics_step(dyn, std::min(every2, slide_steps - done), 0, row, &took, stats));
        CHECK(ctx, fh_obstacle_offsets(ctx, offset, nullptr));
        CHECK(ctx, fh_contact_resultants(ctx, R, nullptr));
        CHECK(ctx, fh_dynamics_state(dyn, nullptr, v.data(), nullptr, nullptr, nullptr));
        double vx = 0.0;
        for (size_t i = 0; i < nv; ++i) vx += v[3 * i] / double(nv);
        std::printf("%10.4f %14.5f %14.5f %14.6f\n", row[3], offset[0], vx, -R[2]);
    }
    std::printf("indented_block3d: kernel %s\n", fh_last_kernel_name(ctx));
    fh_dynamics_destroy(dyn);
    fh_destroy(ctx);
    return 0;
}
