// C++ host, no Python: a torus-shaped die, given as a sampled signed-distance grid, pressed into the top of a clamped block.
//   Unit cube of Hex8, FH_LINEAR_ELASTIC, clamped on its bottom face.  The die is a torus with its axis along z (ring radius 0.3, tube
//   radius 0.1), whose signed distance sqrt((sqrt(x^2 + y^2) - R)^2 + z^2) - r is sampled on the host on a regular grid
//   (fh_sdf_grid_create) over a box that covers the whole block and the die above it, so that no node can leave the box while it touches the
//   die.  The obstacle (FH_OBSTACLE_GRID) places sample (0, 0, 0) at `point`; a path (fh_set_obstacle_paths) moves it: the die rests on the
//   middle of the top face, is pressed in by `depth` over the first half of the run and retracted past its start over the second.  Backward
//   Euler (fh_dynamics_step) moves the contact clock itself; after every record the example prints the time, the indentation
//   (fh_obstacle_offsets) and the force the block exerts on the die, R_o of fh_contact_resultants: the force-indentation curve.
// Build:  make -C examples    Run: ./examples/stamped_block3d [cells_per_unit = 8 [steps = 40 [depth = 0.04 [samples_per_axis = 49]]]]
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
    const uint64_t cpu = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 8;
    const uint64_t steps = argc > 2 ? std::max<uint64_t>(4, std::strtoull(argv[2], nullptr, 10)) : 40;
    const double depth = argc > 3 ? std::strtod(argv[3], nullptr) : 0.04;
    const uint32_t samples = argc > 4 ? (uint32_t)std::max<uint64_t>(9, std::strtoull(argv[4], nullptr, 10)) : 49;
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
    const double k_node = 2e3 * 16.0 / double(cpu * cpu);   // per node: the stiffness per area stays as the mesh is refined

    fh_ctx* ctx = fh_create(0);
    if (!ctx) { std::fprintf(stderr, "no HIP device\n"); return 2; }
    CHECK(ctx, fh_set_mesh(ctx, FH_HEX8, vertices.data(), nv, connectivity.data(), nc));
    CHECK(ctx, fh_set_operator(ctx, FH_LINEAR_ELASTIC));
    CHECK(ctx, fh_set_quadrature_uniform(ctx, w.data(), xi.data(), 8, lame.data()));
    CHECK(ctx, fh_set_mass_density(ctx, &rho, 1));
    std::vector<uint64_t> bottom;
    for (uint64_t i = 0; i < nv; ++i)
        if (vertices[3 * i + 2] == 0.0) bottom.push_back(i);
    CHECK(ctx, fh_set_operator_dirichlet_nodes(ctx, bottom.data(), bottom.size()));

    // the die in its own frame: the torus around the origin, sampled over [-1, 1]^2 x [-1.5, 0.5], x fastest
    const double ring = 0.3, tube = 0.1;
    const double lower[3] = {-1.0, -1.0, -1.5}, extent[3] = {2.0, 2.0, 2.0};
    const uint32_t cnt[3] = {samples, samples, samples};
    double h[3];
    for (int a = 0; a < 3; ++a) h[a] = extent[a] / double(samples - 1);
    std::vector<double> phi((size_t)samples * samples * samples);
    for (uint32_t iz = 0; iz < samples; ++iz)
        for (uint32_t iy = 0; iy < samples; ++iy)
            for (uint32_t ix = 0; ix < samples; ++ix) {
                const double x = lower[0] + ix * h[0], y = lower[1] + iy * h[1], z = lower[2] + iz * h[2];
                const double q = std::sqrt(x * x + y * y) - ring;
                phi[((size_t)iz * samples + iy) * samples + ix] = std::sqrt(q * q + z * z) - tube;
            }
    uint32_t grid = 0;
    CHECK(ctx, fh_sdf_grid_create(ctx, 3, cnt, h, phi.data(), &grid));
    fh_obstacle die{};
    die.kind = FH_OBSTACLE_GRID;
    die.grid = (int)grid;
    die.stiffness = k_node;
    // the torus's centre above the middle of the top face, its lowest circle touching the face: sample (0, 0, 0) goes with it
    const double centre[3] = {0.5, 0.5, 1.0 + tube};
    for (int a = 0; a < 3; ++a) die.point[a] = centre[a] + lower[a];
    CHECK(ctx, fh_set_obstacles(ctx, &die, 1, nullptr));
    fh_dynamics_settings s{};
    s.scheme = FH_DYN_BACKWARD_EULER;
    s.dt = 0.02;
    s.newton_tolerance = 1e-9;
    s.newton_max_iterations = 60;
    s.line_search = FH_NEWTON_BACKTRACKING;
    s.preconditioner = FH_PRECOND_JACOBI;
    s.linear_rel_tol = 1e-10;
    const double T = double(steps) * s.dt;
    const uint64_t knot_begin[2] = {0, 3};
    const double knot_time[3] = {0.0, 0.5 * T, T};
    const double knot_offset[9] = {0.0, 0.0, 0.0, 0.0, 0.0, -depth, 0.0, 0.0, 0.5 * depth};
    CHECK(ctx, fh_set_obstacle_paths(ctx, knot_begin, knot_time, knot_offset));
    fh_dynamics* dyn = nullptr;
    CHECK(ctx, fh_dynamics_create(ctx, &s, &dyn));
    CHECK(ctx, fh_dynamics_set_state(dyn, nullptr, nullptr));
    const uint64_t every = std::max<uint64_t>(1, steps / 10);
    std::printf("stamped_block3d: %llu Hex8 clamped at z = 0, a torus die (%u^3 samples, spacing %.4f) pressed in by %.3f and retracted; backward Euler, dt = %.3f\n",
                (unsigned long long)nc, samples, h[0], depth, s.dt);
    std::printf("%10s %14s %14s %14s\n", "time", "indentation", "force on die", "stored energy");
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
    if (last == 0.0) std::printf("stamped_block3d: peak force %.6f; retracted, the die is clear of the block\n", peak);
    else std::printf("stamped_block3d: peak force %.6f; the block still presses on the retracted die with %.6f\n", peak, last);
    fh_dynamics_destroy(dyn);
    CHECK(ctx, fh_set_obstacles(ctx, nullptr, 0, nullptr));
    CHECK(ctx, fh_sdf_grid_destroy(ctx, grid));
    fh_destroy(ctx);
    return 0;
}
