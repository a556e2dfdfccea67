#!/usr/bin/env python3
"""Jacobi-PCG against MG-PCG under quadratic meshes, the hierarchy ending in the degree coarsening of the fine mesh (fh_coarsen_degree,
fa.degree_hierarchy) over linear levels from the device refiner:

    hex27   Hex27 LinearElastic on 32^3 cells, Hex8 levels 2^3 .. 32^3
    tet10   Tet10 LinearElastic on BCC 20 (96 000 cells: C3's tetrahedra about two levels coarser, at a size that refines from a coarsest
            level the exact solve takes), Tet4 levels BCC 5, 10, 20

One JSON line per config, printed and appended to profiles/degree_multigrid.jsonl: PCG iterations to 1e-8 and the time of the second of
two solves for both preconditioners on one engine; the wall time of fh_coarsen_degree + fh_set_mesh_from_degree_coarsening (median of 5
after a warm-up) beside the sequential sweep of tests/test_degree_coarsening.py on the same mesh, the only other way to this result; the
time of one V-cycle and of one application of the fine operator, which the V-cycle calls six times.  Reported figures: nothing passes or
fails on them.  The kernels by name come from a kernel trace of the same command:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o degree -- python scripts/bench_degree_multigrid.py CONFIG

    python scripts/bench_degree_multigrid.py [hex27 | tet10] [refinements]      defaults: hex27 4; tet10 2
"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fenris_amd as fa  # noqa: E402
from fenris_amd import quadrature  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "degree_multigrid.jsonl")
FINE_APPLIES_PER_VCYCLE = 6   # Chebyshev degree 3 from zero: 2; the residual: 1; Chebyshev degree 3 from the corrected iterate: 3

CONFIGS = {
    "hex27": (lambda: fa.procedural.create_unit_box_uniform_hex_mesh_3d(2), fa.hex27_mesh_from_hex8, lambda: quadrature.tensor.hexahedron_gauss(3), 4,
              "Hex27 LinearElastic on {n} cells over Hex8 levels from 2^3"),
    "tet10": (lambda: fa.procedural.create_unit_box_uniform_tet_mesh_3d(5), fa.tet10_mesh_from_tet4, lambda: quadrature.total_order.tetrahedron(2), 2,
              "Tet10 LinearElastic on {n} cells over Tet4 levels from BCC 5"),
}


def median_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float(np.min(ts))


def timed(fn):
    fn()   # (warm-up: tables, buffers, setup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, 1e3 * (time.perf_counter() - t0)


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "hex27"
    base, convert, rule, levels, title = CONFIGS[which]
    levels = int(sys.argv[2]) if len(sys.argv) > 2 else levels
    lame = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.3))
    w, p = rule()
    qt = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(lame)
    work, lin_eng = fa.Engine(0), fa.Engine(0)
    t0 = time.perf_counter()
    linear, ts = fa.refine_uniformly_repeat_with_transfers(base(), levels, work)
    refine_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    high = convert(linear[-1])
    convert_s = time.perf_counter() - t0
    out = {"config": title.format(n=high.num_elements()) + ", x = 1 clamped, unit load in -y, rel_tol 1e-8", "elements": high.num_elements(),
           "nodes": high.num_nodes(), "levels": len(linear) + 1, "device_refine_s": refine_s, "host_convert_s": convert_s}

    # the p-coarsening step alone: device pass + device-to-device set_mesh, against the sequential sweep
    work.set_mesh(high)

    def device_pair():
        work.coarsen_degree()
        lin_eng.set_mesh_from_degree_coarsening(work)

    out["device_coarsen_set_mesh_ms"], out["device_coarsen_set_mesh_min_ms"] = median_ms(device_pair, 5)
    out["device_coarsen_ms"] = median_ms(work.coarsen_degree, 5)[0]
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_degree_coarsening import sweep  # noqa: E402

    t0 = time.perf_counter()
    swept = sweep(high)
    out["host_sweep_ms"] = 1e3 * (time.perf_counter() - t0)
    lin, pt, vn = work.degree_coarsening()
    out["sweep_identical"] = bool(np.array_equal(swept[2], lin.connectivity) and np.array_equal(swept[5], pt.indices) and np.array_equal(swept[3], vn))
    out["coarse_vertices"], out["transfer_nnz"] = lin.num_nodes(), len(pt.indices)
    t0 = time.perf_counter()
    coarse, transfers = fa.degree_hierarchy(high, linear, ts, work)
    out["degree_hierarchy_s"] = time.perf_counter() - t0
    work.close()
    lin_eng.close()

    eng = fa.Engine(0, stream=torch.cuda.current_stream().cuda_stream)
    n = 3 * high.num_nodes()
    asm = (fa.ElementEllipticAssemblerBuilder(eng).with_finite_element_space(high).with_operator(fa.MaterialEllipticOperator(fa.LinearElasticMaterial()))
           .with_quadrature_table(qt).with_u(None).build())
    bc = np.where(np.isclose(high.vertices[:, 0], 1.0))[0]
    b = torch.zeros(n, dtype=torch.float64, device="cuda")
    b[1::3] = -1.0 / high.num_nodes()
    b[torch.from_numpy(np.repeat(3 * bc, 3) + np.tile(np.arange(3), len(bc))).cuda()] = 0.0
    mg = fa.GeometricMultigrid(asm, coarse, transfers)
    op = fa.MatrixFreeOperator(asm).with_dirichlet_nodes(bc).with_multigrid(mg)
    x = torch.zeros_like(b)
    it_j, t_j = timed(lambda: op.cg_solve(b, x.zero_(), fa.PRECOND_JACOBI, 1e-8))
    xj = x.clone()
    it_m, t_m = timed(lambda: op.cg_solve(b, x.zero_(), fa.PRECOND_MULTIGRID, 1e-8))
    out.update({"jacobi_iterations": it_j, "jacobi_solve_ms": t_j, "mg_iterations": it_m, "mg_solve_ms": t_m, "speedup": t_j / t_m,
                "max_rel_diff_x": float((x - xj).abs().max() / xj.abs().max()),
                "lambda_max_by_level": [mg.level_info(k)[0] for k in range(len(coarse) + 1)]})
    # one V-cycle and one application of the fine operator (the per-element path), 20 of each
    z, y = torch.empty_like(b), torch.empty_like(b)

    def many(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / 20

    mg.apply(b, z, dirichlet_nodes=bc)   # binds the hierarchy to these Dirichlet nodes
    out["vcycle_ms"] = many(lambda: eng._check(fa._ffi.lib().fh_mg_apply_dev(mg._h, 0.0, 1.0, C.c_void_p(b.data_ptr()), C.c_void_p(z.data_ptr()))))
    out["fine_apply_ms"] = many(lambda: eng.apply_operator_dev(b, y))
    out["fine_apply_share_of_vcycle"] = FINE_APPLIES_PER_VCYCLE * out["fine_apply_ms"] / out["vcycle_ms"]
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))
    with open(OUT, "a") as fh:
        fh.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
