#!/usr/bin/env python3
"""Matrix-free shifted tangent alpha M + beta T(u) (fh_apply_shifted_tangent_dev, backward Euler: alpha = 1, beta = dt^2) against the plain
map, one process, one GPU: the plain application (fh_apply_operator_dev for LinearElastic, fh_apply_tangent_dev otherwise), the shifted
one, the mass alone (beta = 0), the shifted diagonal, one Jacobi-PCG iteration (clamped face x = 0) and the device memory the matrix-free
path holds; where the assembled matrices fit (assemble_csr) also one Jacobi-PCG iteration on the assembled alpha M + beta K(u) with
fh_spmv_dev.  One JSON line per config, printed and appended to profiles/shifted.jsonl.

    python scripts/bench_shifted.py CONFIG [cells]     CONFIG: hex8_le | hex8_nh | hex8_nh_csr | tet4_c3 | hex27_nh
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

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "shifted.jsonl")
DT, RHO = 1e-3, 1000.0


def measure(label, mesh, qt, material, bc, assemble_csr, linear):
    out = {"config": label, "elements": mesh.num_elements(), "nodes": mesh.num_nodes(), "alpha": 1.0, "beta": DT * DT}
    alpha, beta = 1.0, DT * DT
    eng = fa.Engine(0, stream=torch.cuda.current_stream().cuda_stream)
    s = mesh.vertices.shape[1]
    n = s * mesh.num_nodes()
    b = torch.zeros(n, dtype=torch.float64, device="cuda")
    b[s - 1::s] = -1.0 / mesh.num_nodes()
    x = torch.randn(n, dtype=torch.float64, device="cuda")
    y = torch.empty_like(x)
    v = torch.from_numpy(mesh.vertices).cuda()
    u = (0.0 * v[:, 0:s] if linear else 0.02 * torch.sin(np.pi * v[:, [1, 2, 0] if s == 3 else [1, 0]])).reshape(-1).contiguous()
    mem0 = used_bytes()
    asm = (fa.ElementEllipticAssemblerBuilder(eng).with_finite_element_space(mesh).with_operator(fa.MaterialEllipticOperator(material))
           .with_quadrature_table(qt).with_u(u).build())
    eng.apply_dirichlet_rhs_dev(b, bc)
    plain = fa.MatrixFreeOperator(asm) if linear else fa.MatrixFreeTangent(asm)
    out["plain_apply_ms"] = ev_time(lambda: plain.apply(y, x))
    out["kernel_plain"] = eng.last_kernel_name()
    plain.with_dirichlet_nodes(bc)

    def plain_solve(k):
        z = torch.zeros(n, dtype=torch.float64, device="cuda")
        plain.cg_solve(b, z, 1, 1e-14, k)
    out["plain_pcg_iteration_ms"] = pcg_ms_per_iteration(plain_solve)
    out["plain_device_bytes"] = used_bytes() - mem0   # (the plain map's own PCG, same process: what the shifted map adds is the difference)
    plain.with_dirichlet_nodes(None)
    sh = fa.MatrixFreeShiftedTangent(asm, RHO, alpha, beta)
    out["shifted_apply_ms"] = ev_time(lambda: sh.apply(y, x))
    out["kernel_shifted"] = eng.last_kernel_name()
    out["shifted_over_plain"] = out["shifted_apply_ms"] / out["plain_apply_ms"]
    mass = fa.MatrixFreeMass(asm, RHO)
    out["mass_apply_ms"] = ev_time(lambda: mass.apply(y, x))
    out["kernel_mass"] = eng.last_kernel_name()
    out["mass_over_plain"] = out["mass_apply_ms"] / out["plain_apply_ms"]
    d = torch.empty_like(x)
    out["shifted_diagonal_ms"] = ev_time(lambda: eng.shifted_tangent_diagonal_dev(alpha, beta, d), steps=5)
    sh.with_dirichlet_nodes(bc)
    sh.apply(y, x)   # (binds density and nodes, forms the scale)

    def mf_solve(k):
        z = torch.zeros(n, dtype=torch.float64, device="cuda")
        eng.cg_solve_shifted_tangent(alpha, beta, b, z, 1, 1e-14, k)
    out["shifted_pcg_iteration_ms"] = pcg_ms_per_iteration(mf_solve)
    out["shifted_device_bytes"] = used_bytes() - mem0
    if assemble_csr:
        mem1 = used_bytes()
        eng.build_pattern()
        kv = torch.zeros(eng.nnz(), dtype=torch.float64, device="cuda")
        eng.assemble_matrix(kv, fa.SCATTER_GATHER | fa.ASSEMBLE_OVERWRITE)
        meng = fa.Engine(0, stream=torch.cuda.current_stream().cuda_stream)
        w, p = qt.weights, qt.points
        mq = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(fa.Density(RHO))
        masm = fa.ElementMassAssembler.with_solution_dim(s, meng).with_space(mesh).with_quadrature_table(mq)
        meng.build_pattern()
        mv = torch.zeros(meng.nnz(), dtype=torch.float64, device="cuda")
        meng.assemble_matrix(mv, fa.SCATTER_GATHER | fa.ASSEMBLE_OVERWRITE)
        values = alpha * mv + beta * kv
        del kv, mv, masm
        meng.close()
        out["spmv_ms"] = ev_time(lambda: eng.spmv(values, x, y))
        eng.apply_dirichlet_csr_dev(values, bc)

        def csr_solve(k):
            z = torch.zeros(n, dtype=torch.float64, device="cuda")
            eng.cg_solve(values, b, z, 1, 1e-14, k)
        out["csr_pcg_iteration_ms"] = pcg_ms_per_iteration(csr_solve)
        out["csr_device_bytes"] = used_bytes() - mem1
        out["pcg_iteration_ratio"] = out["shifted_pcg_iteration_ms"] / out["csr_pcg_iteration_ms"]
        del values
    print(json.dumps(out), flush=True)
    with open(OUT, "a") as f:
        f.write(json.dumps(out) + "\n")
    eng.close()
    torch.cuda.empty_cache()
    return out


def main():
    which = sys.argv[1]
    lame = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.2))
    w, p = quadrature.tensor.hexahedron_gauss(2)
    qt = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(lame)
    if which.startswith("hex8"):
        c = int(sys.argv[2]) if len(sys.argv) > 2 else (128 if which == "hex8_nh_csr" else 216)
        m = fa.procedural.create_unit_box_uniform_hex_mesh_3d(c)
        bc = np.where(m.vertices[:, 0] < 1e-9)[0]
        if which == "hex8_le":
            measure(f"Hex8 LinearElastic {c}^3 (all-affine box), x = 0 clamped", m, qt, fa.LinearElasticMaterial(), bc, False, True)
        else:
            measure(f"Hex8 NeoHookean {c}^3 (all-affine box), u != 0, x = 0 clamped", m, qt, fa.NeoHookeanMaterial(), bc,
                    which == "hex8_nh_csr", False)
        return
    if which == "hex27_nh":   # a quadratic kind: the per-element kernels (k_mf_apply_elements, k_mass_elements)
        c = int(sys.argv[2]) if len(sys.argv) > 2 else 40
        m = fa.hex27_mesh_from_hex8(fa.procedural.create_unit_box_uniform_hex_mesh_3d(c))
        w3, p3 = quadrature.tensor.hexahedron_gauss(3)
        qt3 = fa.UniformQuadratureTable.from_points_and_weights(p3, w3).with_uniform_data(lame)
        measure(f"Hex27 NeoHookean {c}^3, Gauss 3, u != 0, x = 0 clamped", m, qt3, fa.NeoHookeanMaterial(),
                np.where(m.vertices[:, 0] < 1e-9)[0], False, False)
        return
    tet_res = int(sys.argv[2]) if len(sys.argv) > 2 else 75
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
            fa.NeoHookeanMaterial(), np.where(verts[:, 0] < 1e-9)[0], True, False)


if __name__ == "__main__":
    main()
