#!/usr/bin/env python3
"""Matrix-free operator against the assembled CSR path, one process, one GPU: operator application vs fh_spmv_dev, one PCG
iteration both ways (Jacobi, clamped face), setup (tiles + diagonal vs pattern + assembly + inverse diagonal) and the device
memory each path holds (hipMemGetInfo before and after).  Configs: the headline mesh (Hex8 linear elasticity, all-affine box)
and C3's Tet4 mesh (BCC res 75, vertices and elements permuted).  Prints one JSON line per config.

    python scripts/bench_matrix_free.py [cells (216)] [tet_res (75)]
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


def ev_time(fn, steps=10, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def used_bytes():
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    return total - free


def pcg_ms_per_iteration(solve, lo=10, hi=60):
    """(time of hi iterations - time of lo iterations) / (hi - lo): the setup of a solve cancels"""
    def run(k):
        def f():
            try:
                solve(k)
            except fa.CgSolveError as exc:
                assert exc.code == 7, exc   # max iterations reached: what is asked for here
        return f
    run(lo)()   # warm-up
    return (wall(run(hi)) - wall(run(lo))) / (hi - lo)


def measure(label, mesh, qt, bc):
    out = {"config": label, "elements": mesh.num_elements(), "nodes": mesh.num_nodes()}
    eng = fa.Engine(0, stream=torch.cuda.current_stream().cuda_stream)
    s = mesh.vertices.shape[1]
    n = s * mesh.num_nodes()
    b = torch.zeros(n, dtype=torch.float64, device="cuda")
    b[s - 1::s] = -1.0 / mesh.num_nodes()
    x = torch.randn(n, dtype=torch.float64, device="cuda")
    y = torch.empty_like(x)
    mem0 = used_bytes()
    asm = (fa.ElementEllipticAssemblerBuilder(eng).with_finite_element_space(mesh)
           .with_operator(fa.MaterialEllipticOperator(fa.LinearElasticMaterial())).with_quadrature_table(qt)
           .with_u(np.zeros(n)).build())
    eng.apply_dirichlet_rhs_dev(b, bc)
    # ---- matrix-free
    op = fa.MatrixFreeOperator(asm)
    d = torch.empty_like(x)
    out["mf_setup_first_ms"] = wall(lambda: eng.operator_diagonal_dev(d))     # tiles (built once per topology) + diagonal
    out["mf_diagonal_ms"] = ev_time(lambda: eng.operator_diagonal_dev(d), steps=5)
    out["mf_apply_ms"] = ev_time(lambda: op.apply(y, x))
    out["kernel_mf"] = eng.last_kernel_name()

    def mf_solve(k):
        u = torch.zeros(n, dtype=torch.float64, device="cuda")
        eng.cg_solve_matrix_free(b, u, 1, 1e-12, k)
    out["mf_pcg_iteration_no_dirichlet_ms"] = pcg_ms_per_iteration(mf_solve)   # (what the Dirichlet mask costs: the difference)
    op.with_dirichlet_nodes(bc)
    out["mf_pcg_iteration_ms"] = pcg_ms_per_iteration(mf_solve)
    out["mf_device_bytes"] = used_bytes() - mem0
    # ---- assembled
    mem1 = used_bytes()
    t_pat = wall(lambda: eng.build_pattern())
    nnz = eng.nnz()
    values = torch.zeros(nnz, dtype=torch.float64, device="cuda")
    t_asm = wall(lambda: eng.assemble_matrix(values, fa.SCATTER_GATHER | fa.ASSEMBLE_OVERWRITE))
    out["csr_pattern_ms"], out["csr_first_assembly_ms"] = t_pat, t_asm
    out["csr_assembly_ms"] = ev_time(lambda: eng.assemble_matrix(values, fa.SCATTER_GATHER | fa.ASSEMBLE_OVERWRITE), steps=3, warmup=1)
    out["spmv_ms"] = ev_time(lambda: eng.spmv(values, x, y))
    eng.apply_dirichlet_csr_dev(values, bc)

    def csr_solve(k):
        u = torch.zeros(n, dtype=torch.float64, device="cuda")
        eng.cg_solve(values, b, u, 1, 1e-12, k)
    out["csr_pcg_iteration_ms"] = pcg_ms_per_iteration(csr_solve)

    def csr_setup(pre):   # a solve of one iteration: with Jacobi it also forms the inverse diagonal
        def f():
            u = torch.zeros(n, dtype=torch.float64, device="cuda")
            try:
                eng.cg_solve(values, b, u, pre, 1e-12, 1)
            except fa.CgSolveError:
                pass
        return f
    csr_setup(1)()
    out["csr_inverse_diagonal_ms"] = min(wall(csr_setup(1)) for _ in range(5)) - min(wall(csr_setup(0)) for _ in range(5))
    out["csr_device_bytes"] = used_bytes() - mem1
    out["nnz_scalar"] = nnz * s * s
    out["apply_over_spmv"] = out["mf_apply_ms"] / out["spmv_ms"]
    out["pcg_iteration_ratio"] = out["mf_pcg_iteration_ms"] / out["csr_pcg_iteration_ms"]
    print(json.dumps(out), flush=True)
    del values
    eng.close()
    torch.cuda.empty_cache()
    return out


def main():
    cells = int(sys.argv[1]) if len(sys.argv) > 1 else 216
    tet_res = int(sys.argv[2]) if len(sys.argv) > 2 else 75
    lame = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.2))
    w, p = quadrature.tensor.hexahedron_gauss(2)
    m = fa.procedural.create_unit_box_uniform_hex_mesh_3d(cells)
    qt = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(lame)
    measure(f"Hex8 linear elasticity {cells}^3 (all-affine box), x = 0 clamped", m, qt, np.where(m.vertices[:, 0] < 1e-9)[0])
    del m
    t = fa.procedural.create_unit_box_uniform_tet_mesh_3d(tet_res)
    rng = np.random.Generator(np.random.MT19937(12345))   # C3 (scripts/bench_configs.py): vertices and elements permuted
    vp = rng.permutation(t.num_nodes())
    inv = np.empty_like(vp)
    inv[vp] = np.arange(len(vp))
    verts = t.vertices[vp]
    conn = inv[t.connectivity.astype(np.int64)][rng.permutation(t.num_elements())].astype(np.uint64)
    w4, p4 = quadrature.total_order.tetrahedron(1)
    qt4 = fa.UniformQuadratureTable.from_points_and_weights(p4, w4).with_uniform_data(lame)
    measure(f"C3 Tet4 linear elasticity BCC res {tet_res}, permuted, x = 0 clamped", fa.Mesh(verts, conn, fa.TET4), qt4,
            np.where(verts[:, 0] < 1e-9)[0])


if __name__ == "__main__":
    main()
