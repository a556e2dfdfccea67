// C++ host, no Python: a block pressed on a floor by a dead load, seated by augmented-Lagrangian multiplier updates.
//   Unit cube of Hex8, FH_LINEAR_ELASTIC, resting on the floor z >= 0 (fh_set_obstacles) with no other support in z; rollers on the faces
//   x = 0 and y = 0 (fh_set_operator_dirichlet_dofs) take the rigid modes.  A dead load F is spread over the nodes of the top face.
//   With the penalty alone (fh_newton_solve) the block sits F / (k w) per node inside the floor.  Each fh_contact_multiplier_update then
//   adds the penetration it finds to the multipliers, the next solve sees the floor shifted by them, and the penetration falls to below
//   1e-10 at the same, moderate k.  The example prints the penetration per update and, at the end, the resultant on the floor
//   (fh_contact_resultants) against the applied load.
// Build:  make -C examples    Run: ./examples/seated_block3d [cells_per_unit = 4 [load = 2.0 [stiffness_per_node = 1e4]]]
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
    const double load = argc > 2 ? std::strtod(argv[2], nullptr) : 2.0;
    const double k_node = argc > 3 ? std::strtod(argv[3], nullptr) : 1e4;
    const double E = 1e3, nu = 0.3, tol = 1e-10;
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

    fh_ctx* ctx = fh_create(0);
    if (!ctx) { std::fprintf(stderr, "no HIP device\n"); return 2; }
    CHECK(ctx, fh_set_mesh(ctx, FH_HEX8, vertices.data(), nv, connectivity.data(), nc));
    CHECK(ctx, fh_set_operator(ctx, FH_LINEAR_ELASTIC));
    CHECK(ctx, fh_set_quadrature_uniform(ctx, w.data(), xi.data(), 8, lame.data()));

    // rollers: u_x on the face x = 0, u_y on the face y = 0; the dead load on the top face; the bottom face meets the floor
    std::vector<uint64_t> held;
    std::vector<uint8_t> components;
    std::vector<double> f(n, 0.0), u(n, 0.0);
    uint64_t top = 0, bottom = 0;
    for (uint64_t i = 0; i < nv; ++i) {
        const uint8_t mask = (vertices[3 * i] == 0.0 ? 1 : 0) | (vertices[3 * i + 1] == 0.0 ? 2 : 0);
        if (mask) { held.push_back(i); components.push_back(mask); }
        top += vertices[3 * i + 2] == 1.0;
        bottom += vertices[3 * i + 2] == 0.0;
    }
    for (uint64_t i = 0; i < nv; ++i)
        if (vertices[3 * i + 2] == 1.0) f[3 * i + 2] = -load / double(top);
    CHECK(ctx, fh_set_operator_dirichlet_dofs(ctx, held.data(), components.data(), held.size()));
    fh_obstacle floor{};
    floor.kind = FH_OBSTACLE_HALF_SPACE;
    floor.stiffness = k_node;
    floor.normal[2] = 1.0;
    CHECK(ctx, fh_set_obstacles(ctx, &floor, 1, nullptr));
    // the guess: the uniform penetration at which the penalty carries the load (at u = 0 the bottom nodes are ON the floor, inactive)
    const double uniform = load / (k_node * double(bottom));
    for (uint64_t i = 0; i < nv; ++i) u[3 * i + 2] = -uniform;

    std::printf("seated_block3d: %llu Hex8 on the floor z >= 0, dead load %.3f on %llu top nodes, k = %.3g per node: F / (k w) = %.3e over %llu bottom nodes\n",
                (unsigned long long)nc, load, (unsigned long long)top, k_node, uniform, (unsigned long long)bottom);
    std::printf("%8s %8s %16s %16s %10s %16s\n", "update", "newton", "penetration", "max change", "active", "largest force");
    fh_multiplier_update st{};
    double first = 0.0;
    int update = 0;
    for (; update < 30; ++update) {
        uint64_t stats[4];
        double norms[3];
        CHECK(ctx, fh_newton_solve(ctx, 0.0, 1.0, f.data(), nullptr, u.data(), 1e-11, 40, FH_NEWTON_BACKTRACKING, FH_PRECOND_JACOBI, 1e-13, 0, stats, norms));
        CHECK(ctx, fh_contact_multiplier_update(ctx, nullptr, 0, &st));
        if (update == 0) first = st.max_penetration;
        std::printf("%8d %8llu %16.6e %16.6e %10llu %16.6e\n", update, (unsigned long long)stats[0], st.max_penetration, st.max_change,
                    (unsigned long long)st.active, st.max_force);
        if (st.max_change <= tol) break;
    }
    double R[3];
    CHECK(ctx, fh_contact_resultants(ctx, R, nullptr));
    std::printf("seated_block3d: penetration %.3e -> %.3e in %d updates; the floor carries %.10f of the applied %.10f; kernel %s\n", first,
                st.max_penetration, update + 1, -R[2], load, fh_last_kernel_name(ctx));
    fh_destroy(ctx);
    const bool ok = update < 30 && first >= uniform && st.max_penetration <= tol && std::fabs(-R[2] - load) <= 1e-8 * load && st.active == bottom;
    return ok ? 0 : 3;
}
