#!/usr/bin/env python3
"""Central-difference steps per second on the device (fh_dynamics_step, CentralDifference) against the same step composed from the public
calls that existed before it: fh_set_u_dev, fh_assemble_vector_dev and torch element-wise updates on u, v, a, f and the lumped mass.  One
process, one GPU, Hex8 LinearElastic and NeoHookean, the face x = 0 clamped, a body load along +x, dt = 0.5 * 2 / omega_max of
fh_dynamics_stable_dt.  One JSON line per config, printed and appended to profiles/dynamics.jsonl.

    python scripts/bench_dynamics.py [hex8_le | hex8_nh | all] [cells = 128] [steps = 200]
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

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dynamics.jsonl")
RHO = 1000.0


def composed_steps(eng, u, v, a, f, m, free, dt, steps):
    """velocity-Verlet with the residual of fh_assemble_vector_dev: what a caller wrote before fh_dynamics_step"""
    r = torch.empty_like(u)
    for _ in range(steps):
        v = v + 0.5 * dt * a
        u = u + dt * v * free
        eng.set_u(u)
        r.zero_()
        eng.assemble_vector(r)
        a = (f - r) / m * free
        v = v + 0.5 * dt * a
    return u, v, a


def measure(label, cells, material, steps):
    mesh = fa.procedural.create_unit_box_uniform_hex_mesh_3d(cells)
    lame = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.2))
    w, p = quadrature.tensor.hexahedron_gauss(2)
    qt = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(lame)
    eng = fa.Engine(0, stream=torch.cuda.current_stream().cuda_stream)
    n = 3 * mesh.num_nodes()
    bc = np.where(mesh.vertices[:, 0] < 1e-9)[0]
    asm = (fa.ElementEllipticAssemblerBuilder(eng).with_finite_element_space(mesh).with_operator(fa.MaterialEllipticOperator(material))
           .with_quadrature_table(qt).with_u(np.zeros(n)).build())
    f = torch.zeros(n, dtype=torch.float64, device="cuda")
    f[0::3] = 2.0e4 / mesh.num_nodes()
    out = {"config": label, "elements": mesh.num_elements(), "nodes": mesh.num_nodes(), "steps": steps}
    ti = fa.CentralDifference(asm, RHO, 1.0).with_dirichlet_nodes(bc)
    ti.set_state(torch.zeros(n, dtype=torch.float64, device="cuda"))
    omega, dt_crit = ti.stable_dt(30)
    dt = 0.5 * dt_crit
    out["dt"] = dt
    ti.close()
    ti = fa.CentralDifference(asm, RHO, dt).with_dirichlet_nodes(bc).with_load(f)
    ti.set_state(torch.zeros(n, dtype=torch.float64, device="cuda"))
    ti.step(20)   # warm-up: tiles, lumped mass, a_0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rec = ti.step(steps)
    torch.cuda.synchronize()
    out["fused_steps_per_s"] = steps / (time.perf_counter() - t0)
    out["fused_ms_per_step"] = 1e3 / out["fused_steps_per_s"]
    out["kinetic_end"] = float(rec.kinetic[-1])
    u_f = ti.state(device=True)[0].clone()
    ti.close()
    # the composed step, from the same initial state, for the same number of steps in all (so the two ends can be compared)
    m = fa.MatrixFreeMass(asm, RHO).lumped(device=True)
    free = torch.ones(n, dtype=torch.float64, device="cuda")
    for k in range(3):
        free[3 * torch.from_numpy(bc).cuda() + k] = 0.0
    u = torch.zeros(n, dtype=torch.float64, device="cuda")
    v = torch.zeros_like(u)
    eng.set_u(u)
    r = torch.zeros_like(u)
    eng.assemble_vector(r)
    a = (f - r) / m * free
    u, v, a = composed_steps(eng, u, v, a, f, m, free, dt, 20)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    u, v, a = composed_steps(eng, u, v, a, f, m, free, dt, steps)
    torch.cuda.synchronize()
    out["composed_steps_per_s"] = steps / (time.perf_counter() - t0)
    out["composed_ms_per_step"] = 1e3 / out["composed_steps_per_s"]
    out["fused_over_composed"] = out["fused_steps_per_s"] / out["composed_steps_per_s"]
    out["end_state_difference"] = float((u - u_f).abs().max() / u_f.abs().max())
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "a") as fh:
        fh.write(json.dumps(out) + "\n")
    eng.close()
    torch.cuda.empty_cache()
    return out


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "all"
    cells = int(sys.argv[2]) if len(sys.argv) > 2 else 128
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 200
    if which in ("hex8_le", "all"):
        measure(f"Hex8 LinearElastic {cells}^3, central differences, x = 0 clamped", cells, fa.LinearElasticMaterial(), steps)
    if which in ("hex8_nh", "all"):
        measure(f"Hex8 NeoHookean {cells}^3, central differences, x = 0 clamped", cells, fa.NeoHookeanMaterial(), steps)


if __name__ == "__main__":
    main()
