#!/usr/bin/env python3
"""Jacobi-PCG against AMG-PCG (FH_PRECOND_AMG, fa.SmoothedAggregationAMG) on the same assembled matrix: clamped at x = min x
(fh_apply_dirichlet_csr_dev), right-hand side 1 with the clamped rows 0, PCG to 1e-8.  Setup is timed apart from the solve; of two
setups and of two solves the second is timed.  One JSON line per config, printed and appended to profiles/amg.jsonl: iterations, setup
and solve times, the device memory the hierarchy holds, operator complexity and the levels.  The setup's kernels come from a kernel trace
of the same command:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o amg -- python scripts/bench_amg.py CONFIG

    python scripts/bench_amg.py CONFIG      CONFIG: le128 (LinearElastic Hex8 128^3) | c2 (Laplace Hex8 128^3) | c3 (Tet4 BCC res 75, permuted)
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

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "amg.jsonl")


def problem(name):
    if name == "le128":
        m = fa.procedural.create_unit_box_uniform_hex_mesh_3d(128)
        return m, fa.MaterialEllipticOperator(fa.LinearElasticMaterial()), quadrature.tensor.hexahedron_gauss(2), 0.3, "rigid_body"
    if name == "c2":
        return fa.procedural.create_unit_box_uniform_hex_mesh_3d(128), fa.LaplaceOperator(), quadrature.tensor.hexahedron_gauss(2), None, "constant"
    if name == "c3":   # the C3 mesh of scripts/bench_configs.py
        m = fa.procedural.create_unit_box_uniform_tet_mesh_3d(75)
        rng = np.random.Generator(np.random.MT19937(12345))
        vp = rng.permutation(m.num_nodes())
        inv = np.empty_like(vp)
        inv[vp] = np.arange(len(vp))
        conn = inv[m.connectivity.astype(np.int64)][rng.permutation(m.num_elements())].astype(np.uint64)
        m = fa.Mesh(m.vertices[vp], conn, fa.TET4)
        return m, fa.MaterialEllipticOperator(fa.LinearElasticMaterial()), quadrature.total_order.tetrahedron(1), 0.2, "rigid_body"
    raise SystemExit(__doc__)


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "le128"
    m, op, (w, pts), nu, ns = problem(name)
    s = 1 if nu is None else 3
    qt = fa.UniformQuadratureTable.from_points_and_weights(pts, w)
    if nu is not None:
        qt = qt.with_uniform_data(fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, nu)))
    eng = fa.Engine(0)
    asm = (fa.ElementEllipticAssemblerBuilder(eng).with_finite_element_space(m).with_operator(op).with_quadrature_table(qt)
           .with_u(np.zeros(s * m.num_nodes())).build())
    csr = fa.CsrAssembler(fa.SCATTER_GATHER).assemble(asm, device_values=True)
    x0 = m.vertices[:, 0]
    clamp = np.where(np.isclose(x0, x0.min()))[0].astype(np.uint64)
    eng.apply_dirichlet_csr_dev(csr.values, clamp)
    n = s * m.num_nodes()
    b = torch.ones(n, dtype=torch.float64, device="cuda")
    b[torch.from_numpy((s * clamp.astype(np.int64)[:, None] + np.arange(s)).ravel()).cuda()] = 0.0

    def solve(pre):
        out = []
        for _ in range(2):
            x = torch.zeros_like(b)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            it = eng.cg_solve(csr.values, b, x, pre, 1e-8)
            torch.cuda.synchronize()
            out.append((it, time.perf_counter() - t0))
        return out[-1]

    jac_it, jac_s = solve(fa.PRECOND_JACOBI)
    before = free_bytes()
    amg = fa.SmoothedAggregationAMG(asm, csr, near_nullspace=ns)
    mem = before - free_bytes()
    amg.close()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    amg = fa.SmoothedAggregationAMG(asm, csr, near_nullspace=ns)
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t0
    amg_it, amg_s = solve(fa.PRECOND_AMG)
    levels = [amg.level_info(l) for l in range(amg.num_levels)]
    rec = {"config": name, "dofs": n, "jacobi": {"iterations": jac_it, "solve_ms": 1e3 * jac_s},
           "amg": {"iterations": amg_it, "setup_ms": 1e3 * setup_s, "solve_ms": 1e3 * amg_s, "setup_plus_solve_ms": 1e3 * (setup_s + amg_s),
                   "memory_bytes": int(mem), "operator_complexity": amg.operator_complexity(),
                   "levels": [(lv["num_dofs"], lv["nnz_blocks"], lv["block_size"], lv["lambda_max"]) for lv in levels]}}
    amg.close()
    eng.close()
    line = json.dumps(rec)
    print(line)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
