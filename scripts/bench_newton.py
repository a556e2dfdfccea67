#!/usr/bin/env python3
"""Device Newton solve (fh_newton_solve_dev, MatrixFreeNewton) against the same loop composed in Python from the existing entry points
(fh_assemble_vector_dev + torch vector ops + fh_set_u_dev + fh_cg_solve_shifted_tangent_dev), one process, one GPU: the whole solve, its
Newton iterations, residual evaluations and PCG iterations.  One JSON line per config, printed and appended to profiles/newton.jsonl.  What
one residual evaluation costs in kernels (k_element_pass_tiled, k_mass_tiled, k_newton_from_partials against the composed loop's
k_vector_from_partials and torch's vector kernels) comes from a kernel trace of the same command:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o newton -- python scripts/bench_newton.py CONFIG [cells]

    python scripts/bench_newton.py CONFIG [cells]     CONFIG: hex8_nh | hex8_nh_implicit | tet4_nh
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fenris_amd as fa  # noqa: E402
from fenris_amd import quadrature  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "newton.jsonl")
DT, RHO, LOAD = 1e-2, 1000.0, -2e4


def composed_solve(eng, alpha, beta, f, u_ref, bc_rows, u, tol, rel_tol):
    """newton_line_search with backtracking, composed from the existing entry points; returns (iterations, evaluations, pcg iterations)"""
    n = len(u)
    r = torch.empty_like(u)
    md = torch.empty_like(u)

    def residual():
        eng.set_u(u)
        r.zero_()
        eng.assemble_vector(r)
        F = beta * (r - f)
        if alpha != 0.0:
            eng.apply_shifted_tangent_dev(1.0, 0.0, u - u_ref, md)   # M d (its Dirichlet rows are zeroed below)
            F += alpha * md
        F[bc_rows] = 0.0
        return F, float(torch.linalg.norm(F))

    F, fn = residual()
    it, ev, cg = 0, 1, 0
    q = torch.zeros(n, dtype=torch.float64, device=u.device)
    while fn > tol:
        q.zero_()
        eng.set_u(u)
        cg += eng.cg_solve_shifted_tangent(alpha, beta, F, q, 1, rel_tol, 0)
        g0, a_prev, a = 0.5 * fn * fn, 0.0, 1.0
        while True:
            u -= (a - a_prev) * q
            F, fn = residual()
            ev += 1
            if 0.5 * fn * fn <= (1 - 1e-4 * a) * g0 or a < 1e-6:
                break
            a_prev, a = a, {1.0: 0.75, 0.75: 0.5, 0.5: 0.25}.get(a, 0.25 * a)
        it += 1
    return it, ev, cg


def measure(label, mesh, qt, implicit):
    out = {"config": label, "elements": mesh.num_elements(), "nodes": mesh.num_nodes()}
    eng = fa.Engine(0, stream=torch.cuda.current_stream().cuda_stream)
    s = mesh.vertices.shape[1]
    n = s * mesh.num_nodes()
    x = mesh.vertices
    bc = np.where(x[:, 0] < 1e-9)[0]
    bc_rows = torch.from_numpy(np.repeat(s * bc, s) + np.tile(np.arange(s), len(bc))).cuda()
    face = np.where(x[:, 0] > 1 - 1e-9)[0]
    f = torch.zeros(n, dtype=torch.float64, device="cuda")
    f[torch.from_numpy(s * face).cuda()] = LOAD / len(face)
    asm = (fa.ElementEllipticAssemblerBuilder(eng).with_finite_element_space(mesh).with_operator(fa.MaterialEllipticOperator(fa.NeoHookeanMaterial()))
           .with_quadrature_table(qt).with_u(torch.zeros(n, dtype=torch.float64, device="cuda")).build())
    alpha, beta = (1.0, DT * DT) if implicit else (0.0, 1.0)
    u_ref = torch.zeros(n, dtype=torch.float64, device="cuda")
    solver = fa.MatrixFreeNewton(asm).with_dirichlet_nodes(bc).with_load(f)
    if implicit:
        u_ref[0::s] = 1e-3 * torch.from_numpy(x[:, 0]).cuda()
        u_ref[bc_rows] = 0.0
        solver.with_inertia(RHO, alpha, beta, u_ref)
    u = torch.zeros(n, dtype=torch.float64, device="cuda")
    res = solver.solve(u.clone(), fa.NewtonSettings(50, 1e300))
    tol = 1e-6 * res.initial_residual_norm
    out.update({"alpha": alpha, "beta": beta, "tolerance": tol})
    res = solver.solve(u.clone(), fa.NewtonSettings(50, tol))   # (warm-up: tables, buffers)
    t0 = time.perf_counter()
    uu = u.clone()
    res = solver.solve(uu, fa.NewtonSettings(50, tol))
    torch.cuda.synchronize()
    out["solve_ms"] = 1e3 * (time.perf_counter() - t0)
    out.update({"newton_iterations": res.iterations, "residual_evaluations": res.residual_evaluations, "pcg_iterations": res.linear_iterations,
                "residual_norm": res.residual_norm})
    out["kernel_evaluation"] = eng.last_kernel_name()
    # the composed loop (its Dirichlet nodes and density bound like the solver's)
    solver._bind(force=True)   # (the solver's Dirichlet nodes and density stay bound)
    uc = u.clone()
    composed_solve(eng, alpha, beta, f, u_ref, bc_rows, uc.clone(), tol, 1e-8)   # (warm-up)
    t0 = time.perf_counter()
    it, ev, cg = composed_solve(eng, alpha, beta, f, u_ref, bc_rows, uc, tol, 1e-8)
    torch.cuda.synchronize()
    out["composed_solve_ms"] = 1e3 * (time.perf_counter() - t0)
    out.update({"composed_newton_iterations": it, "composed_residual_evaluations": ev, "composed_pcg_iterations": cg})

    out["max_abs_diff_u"] = float((uu - uc).abs().max())
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))
    with open(OUT, "a") as fh:
        fh.write(json.dumps(out) + "\n")


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "hex8_nh"
    lame = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.3))
    if which in ("hex8_nh", "hex8_nh_implicit"):
        c = int(sys.argv[2]) if len(sys.argv) > 2 else 128
        m = fa.procedural.create_unit_box_uniform_hex_mesh_3d(c)
        w, p = quadrature.tensor.hexahedron_gauss(2)
        qt = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(lame)
        kind = "implicit step" if which == "hex8_nh_implicit" else "static"
        measure(f"Hex8 NeoHookean {c}^3, compressive load, x = 0 clamped, {kind}", m, qt, which == "hex8_nh_implicit")
        return
    c = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    t = fa.procedural.create_unit_box_uniform_tet_mesh_3d(c)
    w, p = quadrature.total_order.tetrahedron(2)
    qt = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(lame)
    measure(f"Tet4 NeoHookean res {c}, compressive load, x = 0 clamped, static", t, qt, False)


if __name__ == "__main__":
    main()
