#!/usr/bin/env python3
"""Jacobi-PCG against MG-PCG (FH_PRECOND_MULTIGRID, fa.GeometricMultigrid) on the same fine mesh: a unit box of 2^3 Hex8 cells refined
uniformly to the fine size, every level renumbered with reorder_mesh_par and its transfers permuted to match.  One JSON line per config,
printed and appended to profiles/multigrid.jsonl: PCG iterations, solve times, the device memory the hierarchy holds.  The V-cycle's
kernels by level come from a kernel trace of the same command (the coarse levels' kernels have the same names; their launch sizes tell
the levels apart):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o mg -- python scripts/bench_multigrid.py CONFIG

    python scripts/bench_multigrid.py CONFIG [cells]     CONFIG: le | hex8_nh | hex8_nh_implicit   (cells: 64 or 128, a power of 2)
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

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "multigrid.jsonl")
DT, RHO, LOAD = 1e-2, 1000.0, -2e4


def hierarchy(cells):
    """meshes (coarsest first) and transfers, every level renumbered"""
    levels = int(round(np.log2(cells))) - 1
    meshes, ts = fa.refine_uniformly_repeat_with_transfers(fa.procedural.create_unit_box_uniform_hex_mesh_3d(2), levels)
    perms = [fa.reorder.reorder_mesh_par(m) for m in meshes]
    meshes = [p.apply(m) for p, m in zip(perms, meshes)]
    ts = [fa.permute_transfer(t, perms[k + 1].vertex_permutation(), perms[k].vertex_permutation()) for k, t in enumerate(ts)]
    return meshes, ts


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def timed(fn):
    fn()   # (warm-up: tables, buffers, setup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, 1e3 * (time.perf_counter() - t0)


def linear(cells, meshes, ts, qt):
    fine = meshes[-1]
    eng = fa.Engine(0, stream=torch.cuda.current_stream().cuda_stream)
    n = 3 * fine.num_nodes()
    asm = (fa.ElementEllipticAssemblerBuilder(eng).with_finite_element_space(fine).with_operator(fa.MaterialEllipticOperator(fa.LinearElasticMaterial()))
           .with_quadrature_table(qt).with_u(None).build())
    bc = np.where(fine.vertices[:, 0] < 1e-9)[0]
    b = torch.zeros(n, dtype=torch.float64, device="cuda")
    b[1::3] = -1.0 / fine.num_nodes()
    b[torch.from_numpy(np.repeat(3 * bc, 3) + np.tile(np.arange(3), len(bc))).cuda()] = 0.0
    before = free_bytes()
    mg = fa.GeometricMultigrid(asm, meshes[:-1], ts)
    op = fa.MatrixFreeOperator(asm).with_dirichlet_nodes(bc).with_multigrid(mg)
    out = {"config": f"Hex8 LinearElastic {cells}^3 (refined from 2^3, renumbered), x = 0 clamped, unit load in -y, rel_tol 1e-8",
           "elements": fine.num_elements(), "nodes": fine.num_nodes(), "levels": len(meshes)}
    x = torch.zeros_like(b)
    it_j, t_j = timed(lambda: op.cg_solve(b, x.zero_(), fa.PRECOND_JACOBI, 1e-8))
    xj = x.clone()
    it_m, t_m = timed(lambda: op.cg_solve(b, x.zero_(), fa.PRECOND_MULTIGRID, 1e-8))
    out["mg_device_bytes"] = before - free_bytes()
    out.update({"jacobi_iterations": it_j, "jacobi_solve_ms": t_j, "mg_iterations": it_m, "mg_solve_ms": t_m, "speedup": t_j / t_m,
                "max_rel_diff_x": float((x - xj).abs().max() / xj.abs().max()),
                "lambda_max_by_level": [mg.level_info(k)[0] for k in range(len(meshes))]})
    return out


def newton(cells, meshes, ts, qt, implicit):
    fine = meshes[-1]
    eng = fa.Engine(0, stream=torch.cuda.current_stream().cuda_stream)
    n = 3 * fine.num_nodes()
    x = fine.vertices
    bc = np.where(x[:, 0] < 1e-9)[0]
    bc_rows = torch.from_numpy(np.repeat(3 * bc, 3) + np.tile(np.arange(3), len(bc))).cuda()
    face = np.where(x[:, 0] > 1 - 1e-9)[0]
    f = torch.zeros(n, dtype=torch.float64, device="cuda")
    f[torch.from_numpy(3 * face).cuda()] = LOAD / len(face)
    asm = (fa.ElementEllipticAssemblerBuilder(eng).with_finite_element_space(fine).with_operator(fa.MaterialEllipticOperator(fa.NeoHookeanMaterial()))
           .with_quadrature_table(qt).with_u(torch.zeros(n, dtype=torch.float64, device="cuda")).build())
    alpha, beta = (1.0, DT * DT) if implicit else (0.0, 1.0)
    solver = fa.MatrixFreeNewton(asm).with_dirichlet_nodes(bc).with_load(f)
    if implicit:
        u_ref = torch.zeros(n, dtype=torch.float64, device="cuda")
        u_ref[0::3] = 1e-3 * torch.from_numpy(x[:, 0]).cuda()
        u_ref[bc_rows] = 0.0
        solver.with_inertia(RHO, alpha, beta, u_ref)
    u = torch.zeros(n, dtype=torch.float64, device="cuda")
    res = solver.solve(u.clone(), fa.NewtonSettings(50, 1e300), preconditioner=fa.PRECOND_JACOBI)
    tol = 1e-6 * res.initial_residual_norm
    kind = "implicit step" if implicit else "static"
    out = {"config": f"Hex8 NeoHookean {cells}^3 (refined from 2^3, renumbered), compressive load, x = 0 clamped, {kind}",
           "elements": fine.num_elements(), "nodes": fine.num_nodes(), "levels": len(meshes), "tolerance": tol}
    uj = u.clone()
    rj, t_j = timed(lambda: solver.solve(uj.copy_(u), fa.NewtonSettings(50, tol), preconditioner=fa.PRECOND_JACOBI))
    before = free_bytes()
    for coarse in ("tangent", "linearized"):
        mg = fa.GeometricMultigrid(asm, meshes[:-1], ts, coarse_operator=coarse)
        solver.with_multigrid(mg)
        um = u.clone()
        rm, t_m = timed(lambda: solver.solve(um.copy_(u), fa.NewtonSettings(50, tol), preconditioner=fa.PRECOND_MULTIGRID))
        out[f"mg_{coarse}"] = {"newton_iterations": rm.iterations, "residual_evaluations": rm.residual_evaluations,
                               "pcg_iterations": rm.linear_iterations, "solve_ms": t_m, "speedup": t_j / t_m,
                               "max_rel_diff_u": float((um - uj).abs().max() / uj.abs().max())}
        if coarse == "tangent":
            out["mg_device_bytes"] = before - free_bytes()
        del mg
    out["jacobi"] = {"newton_iterations": rj.iterations, "residual_evaluations": rj.residual_evaluations, "pcg_iterations": rj.linear_iterations,
                     "solve_ms": t_j}
    return out


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "le"
    cells = int(sys.argv[2]) if len(sys.argv) > 2 else 128
    lame = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.3))
    w, p = quadrature.tensor.hexahedron_gauss(2)
    qt = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(lame)
    t0 = time.perf_counter()
    meshes, ts = hierarchy(cells)
    setup_s = time.perf_counter() - t0
    out = linear(cells, meshes, ts, qt) if which == "le" else newton(cells, meshes, ts, qt, which == "hex8_nh_implicit")
    out["host_refine_reorder_s"] = setup_s
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))
    with open(OUT, "a") as fh:
        fh.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
