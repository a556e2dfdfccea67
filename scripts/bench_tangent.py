#!/usr/bin/env python3
"""Matrix-free tangent T(u) (fh_apply_tangent_dev) against the residual and the assembled K(u), one process, one GPU, u != 0:
one tangent application vs one residual (fh_assemble_vector_dev), the tangent's diagonal, one Jacobi-PCG iteration (clamped face x = 0)
and the device memory the matrix-free path holds; where the assembled tangent fits (assemble_csr=True) also tangent assembly + SpMV
and a PCG iteration on it.  Configs: Hex8 NeoHookean and StVK (all-affine box), C3's permuted Tet4 mesh with NeoHookean.  One JSON
line per config, printed and appended to profiles/tangent.jsonl.

    python scripts/bench_tangent.py [cells (216)] [csr_cells (128)] [tet_res (75)]
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fenris_amd as fa  # noqa: E402
from fenris_amd import quadrature  # noqa: E402
from scripts.bench_matrix_free import ev_time, pcg_ms_per_iteration, used_bytes, wall  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "tangent.jsonl")


def measure(label, mesh, qt, material, bc, assemble_csr):
    out = {"config": label, "elements": mesh.num_elements(), "nodes": mesh.num_nodes()}
    eng = fa.Engine(0, stream=torch.cuda.current_stream().cuda_stream)
    s = mesh.vertices.shape[1]
    n = s * mesh.num_nodes()
    b = torch.zeros(n, dtype=torch.float64, device="cuda")
    b[s - 1::s] = -1.0 / mesh.num_nodes()
    x = torch.randn(n, dtype=torch.float64, device="cuda")
    y = torch.empty_like(x)
    # a smooth deformation (J > 0): u = 0.02 (sin pi x, sin pi y, sin pi z) in every component
    v = torch.from_numpy(mesh.vertices).cuda()
    u = (0.02 * torch.sin(np.pi * v[:, [1, 2, 0] if s == 3 else [1, 0]])).reshape(-1).contiguous()
    mem0 = used_bytes()
    asm = (fa.ElementEllipticAssemblerBuilder(eng).with_finite_element_space(mesh).with_operator(fa.MaterialEllipticOperator(material))
           .with_quadrature_table(qt).with_u(u).build())
    eng.apply_dirichlet_rhs_dev(b, bc)
    r = torch.empty_like(x)
    out["residual_ms"] = ev_time(lambda: eng.assemble_vector(r))
    out["kernel_residual"] = eng.last_kernel_name()
    t = fa.MatrixFreeTangent(asm)
    d = torch.empty_like(x)
    out["tangent_setup_first_ms"] = wall(lambda: eng.tangent_diagonal_dev(d))
    out["tangent_diagonal_ms"] = ev_time(lambda: eng.tangent_diagonal_dev(d), steps=5)
    out["tangent_apply_ms"] = ev_time(lambda: t.apply(y, x))
    out["kernel_tangent"] = eng.last_kernel_name()
    out["apply_over_residual"] = out["tangent_apply_ms"] / out["residual_ms"]
    t.with_dirichlet_nodes(bc)

    def mf_solve(k):
        z = torch.zeros(n, dtype=torch.float64, device="cuda")
        eng.cg_solve_tangent(b, z, 1, 1e-12, k)
    out["tangent_pcg_iteration_ms"] = pcg_ms_per_iteration(mf_solve)
    out["tangent_device_bytes"] = used_bytes() - mem0
    if assemble_csr:
        mem1 = used_bytes()
        eng.build_pattern()
        values = torch.zeros(eng.nnz(), dtype=torch.float64, device="cuda")
        out["csr_tangent_assembly_ms"] = ev_time(lambda: eng.assemble_matrix(values, fa.SCATTER_GATHER | fa.ASSEMBLE_OVERWRITE), steps=3, warmup=1)
        out["kernel_csr"] = eng.last_kernel_name()
        out["spmv_ms"] = ev_time(lambda: eng.spmv(values, x, y))
        out["csr_assembly_plus_spmv_ms"] = out["csr_tangent_assembly_ms"] + out["spmv_ms"]
        eng.apply_dirichlet_csr_dev(values, bc)

        def csr_solve(k):
            z = torch.zeros(n, dtype=torch.float64, device="cuda")
            eng.cg_solve(values, b, z, 1, 1e-12, k)
        out["csr_pcg_iteration_ms"] = pcg_ms_per_iteration(csr_solve)
        out["csr_device_bytes"] = used_bytes() - mem1
        out["pcg_iteration_ratio"] = out["tangent_pcg_iteration_ms"] / out["csr_pcg_iteration_ms"]
        del values
    print(json.dumps(out), flush=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(out) + "\n")
    eng.close()
    torch.cuda.empty_cache()
    return out


def main():
    cells = int(sys.argv[1]) if len(sys.argv) > 1 else 216
    csr_cells = int(sys.argv[2]) if len(sys.argv) > 2 else 128
    tet_res = int(sys.argv[3]) if len(sys.argv) > 3 else 75
    lame = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.2))
    w, p = quadrature.tensor.hexahedron_gauss(2)
    qt = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(lame)
    for c, csr in ((cells, False), (csr_cells, True)):
        m = fa.procedural.create_unit_box_uniform_hex_mesh_3d(c)
        bc = np.where(m.vertices[:, 0] < 1e-9)[0]
        measure(f"Hex8 NeoHookean {c}^3 (all-affine box), u != 0, x = 0 clamped", m, qt, fa.NeoHookeanMaterial(), bc, csr)
        if not csr:
            measure(f"Hex8 StVK {c}^3 (all-affine box), u != 0, x = 0 clamped", m, qt, fa.StVKMaterial(), bc, csr)
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
    measure(f"C3 Tet4 NeoHookean BCC res {tet_res}, permuted, u != 0, x = 0 clamped", fa.Mesh(verts, conn, fa.TET4), qt4,
            fa.NeoHookeanMaterial(), np.where(verts[:, 0] < 1e-9)[0], True)


if __name__ == "__main__":
    main()
