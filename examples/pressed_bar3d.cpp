// C++ host, no Python: a Hex8 bar clamped at one end and pulled at the other by a surface pressure.
//   mesh generator -> boundary search on the device (fh_find_boundary_faces) -> the clamped nodes are the boundary vertices at x = 0,
//   the loaded faces the boundary faces at x = L -> surface load vector (fh_assemble_surface_load_dev) -> stiffness assembly ->
//   homogeneous Dirichlet conditions -> Jacobi-preconditioned CG.  No node or face list comes from anywhere but the search.
// Mirrors a fenris application that calls Mesh::find_boundary_vertices / find_boundary_faces (src/mesh.rs:167-216) for its
// boundary conditions.  cantilever3d.cpp is the body-force counterpart.
// With `stable-neo-hookean` as the second argument the material is FH_STABLE_NEO_HOOKEAN with converted parameters: its tangent at u = 0 is
// the same linear elasticity, so this first Newton step gives the same displacement.
// Build:  make -C examples    Run: ./examples/pressed_bar3d [cells_per_unit [stable-neo-hookean]]
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    const uint64_t cpu = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 8;
    const double L = 4.0, E = 1e7, nu = 0.3, pull = 1e4;   // bar 4 x 1 x 1, pressure -pull on the end face: tension
    uint64_t nv = 0, nc = 0;
    fh_hex_mesh(1.0, 4, 1, 1, cpu, nullptr, nullptr, &nv, &nc);
    std::vector<double> vertices(3 * nv);
    std::vector<uint64_t> connectivity(8 * nc);
    fh_hex_mesh(1.0, 4, 1, 1, cpu, vertices.data(), connectivity.data(), &nv, &nc);
    std::vector<double> w(8), xi(24), wf(4), xf(8);
    fh_hexahedron_gauss(2, w.data(), xi.data());
    fh_quadrilateral_gauss(2, wf.data(), xf.data());   // the face rule on [-1, 1]^2
    double mu, lambda;
    fh_lame_from_young_poisson(E, nu, &mu, &lambda);
    const bool snh = argc > 2 && std::strcmp(argv[2], "stable-neo-hookean") == 0;
    if (snh) fh_stable_neo_hookean_parameters(3, mu, lambda, &mu, &lambda);
    std::vector<double> lame(16);
    for (int q = 0; q < 8; ++q) { lame[2 * q] = mu; lame[2 * q + 1] = lambda; }

    fh_ctx* ctx = fh_create(0);
    if (!ctx) { std::fprintf(stderr, "no HIP device\n"); return 2; }
    CHECK(ctx, fh_set_mesh(ctx, FH_HEX8, vertices.data(), nv, connectivity.data(), nc));
    CHECK(ctx, fh_set_operator(ctx, snh ? FH_STABLE_NEO_HOOKEAN : FH_LINEAR_ELASTIC));
    CHECK(ctx, fh_set_quadrature_uniform(ctx, w.data(), xi.data(), 8, lame.data()));
    CHECK(ctx, fh_set_u(ctx, nullptr));

    // the boundary, from the connectivity alone
    uint64_t num_faces = 0, num_bv = 0;
    uint32_t nf = 0;
    CHECK(ctx, fh_find_boundary_faces(ctx, &num_faces, &nf));
    std::vector<uint64_t> face_nodes(num_faces * nf), cells(num_faces);
    std::vector<uint32_t> local_faces(num_faces);
    CHECK(ctx, fh_boundary_faces(ctx, face_nodes.data(), cells.data(), local_faces.data()));
    CHECK(ctx, fh_boundary_vertices(ctx, &num_bv, nullptr));
    std::vector<uint64_t> bv(num_bv), clamped;
    CHECK(ctx, fh_boundary_vertices(ctx, &num_bv, bv.data()));
    for (uint64_t i : bv)
        if (vertices[3 * i] < 1e-12) clamped.push_back(i);
    std::vector<uint64_t> end_cells;
    std::vector<uint32_t> end_faces;
    for (uint64_t f = 0; f < num_faces; ++f) {
        bool at_end = true;
        for (uint32_t a = 0; a < nf; ++a) at_end = at_end && vertices[3 * face_nodes[f * nf + a]] > L - 1e-12;
        if (at_end) { end_cells.push_back(cells[f]); end_faces.push_back(local_faces[f]); }
    }

    const uint64_t n = 3 * nv;
    std::vector<uint64_t> row_offsets(n + 1);
    uint64_t nnz = 0;
    CHECK(ctx, fh_pattern(ctx, row_offsets.data(), &nnz));
    double *values = nullptr, *rhs = nullptr, *u = nullptr, *p_dev = nullptr;
    uint64_t* ec_dev = nullptr;
    uint32_t* ef_dev = nullptr;
    HIP(hipMalloc(&values, sizeof(double) * nnz));
    HIP(hipMalloc(&rhs, sizeof(double) * n));
    HIP(hipMalloc(&u, sizeof(double) * n));
    HIP(hipMalloc(&p_dev, sizeof(double)));
    HIP(hipMalloc(&ec_dev, sizeof(uint64_t) * end_cells.size()));
    HIP(hipMalloc(&ef_dev, sizeof(uint32_t) * end_faces.size()));
    HIP(hipMemset(rhs, 0, sizeof(double) * n));
    HIP(hipMemset(u, 0, sizeof(double) * n));
    const double p = -pull;
    HIP(hipMemcpy(p_dev, &p, sizeof(double), hipMemcpyHostToDevice));
    HIP(hipMemcpy(ec_dev, end_cells.data(), sizeof(uint64_t) * end_cells.size(), hipMemcpyHostToDevice));
    HIP(hipMemcpy(ef_dev, end_faces.data(), sizeof(uint32_t) * end_faces.size(), hipMemcpyHostToDevice));
    CHECK(ctx, fh_assemble_surface_load_dev(ctx, FH_LOAD_PRESSURE, 3, ec_dev, ef_dev, end_cells.size(), wf.data(), xf.data(), 4, p_dev, 1, rhs));
    uint64_t failed = 0;
    CHECK(ctx, fh_assemble_matrix_dev(ctx, values, FH_SCATTER_GATHER | FH_ASSEMBLE_OVERWRITE, &failed));
    std::vector<double> fh(n);
    CHECK(ctx, fh_synchronize(ctx));
    HIP(hipMemcpy(fh.data(), rhs, sizeof(double) * n, hipMemcpyDeviceToHost));
    CHECK(ctx, fh_apply_dirichlet_csr_dev(ctx, values, clamped.data(), clamped.size()));
    CHECK(ctx, fh_apply_dirichlet_rhs_dev(ctx, rhs, clamped.data(), clamped.size()));
    uint64_t iterations = 0;
    CHECK(ctx, fh_cg_solve_dev(ctx, values, rhs, u, FH_PRECOND_JACOBI, 1e-10, 20000, &iterations));

    std::vector<double> uh(n);
    HIP(hipMemcpy(uh.data(), u, sizeof(double) * n, hipMemcpyDeviceToHost));
    double tip = 0.0, total_load = 0.0, clamped_motion = 0.0;
    uint64_t tip_nodes = 0;
    for (uint64_t i = 0; i < nv; ++i) {
        if (vertices[3 * i] > L - 1e-12) { tip += uh[3 * i]; ++tip_nodes; }
        total_load += fh[3 * i];
    }
    tip /= (double)tip_nodes;
    for (uint64_t i : clamped) clamped_motion = std::fmax(clamped_motion, std::fabs(uh[3 * i]) + std::fabs(uh[3 * i + 1]) + std::fabs(uh[3 * i + 2]));
    const double uniaxial = pull * L / E;   // the clamp stiffens the bar a little: the mean end displacement stays just below it
    std::printf("Hex8 bar %llux%llux%llu pulled on x = %g: %llu boundary faces (%zu loaded), %llu boundary vertices (%zu clamped), "
                "CG iterations %llu, mean end displacement %.6e (uniaxial p L / E %.6e), sum of nodal loads %.10g (p A = %g), "
                "clamped face moves %.1e\n",
                (unsigned long long)(4 * cpu), (unsigned long long)cpu, (unsigned long long)cpu, L, (unsigned long long)num_faces,
                end_cells.size(), (unsigned long long)num_bv, clamped.size(), (unsigned long long)iterations, tip, uniaxial, total_load, pull,
                clamped_motion);
    // the stress of the solution: von Mises per element (fh_recover), its maximum beside the applied traction
    CHECK(ctx, fh_set_u_dev(ctx, u));
    std::vector<double> von_mises(nc);
    CHECK(ctx, fh_recover(ctx, FH_RECOVER_VON_MISES, FH_AT_ELEMENTS, von_mises.data()));
    double vm_max = 0.0;
    for (double s : von_mises) vm_max = std::fmax(vm_max, s);
    std::printf("von Mises stress, maximum over the elements: %.6e (applied traction %g)\n", vm_max, pull);
    (void)hipFree(values); (void)hipFree(rhs); (void)hipFree(u); (void)hipFree(p_dev); (void)hipFree(ec_dev); (void)hipFree(ef_dev);
    fh_destroy(ctx);
    const bool ok = vm_max > 0.5 * pull && iterations > 0 && clamped_motion == 0.0 && end_cells.size() == cpu * cpu && clamped.size() == (cpu + 1) * (cpu + 1) &&
                    std::fabs(total_load - pull) < 1e-9 * pull && tip > 0.9 * uniaxial && tip < 1.001 * uniaxial;
    return ok ? 0 : 3;
}
