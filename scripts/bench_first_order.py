#!/usr/bin/env python3
"""Runge-Kutta-Legendre stages per second on the device (fh_dynamics_step on a handle of fh_first_order_create, RungeKuttaLegendre) against
the same scheme composed from the public calls that existed before it: fh_set_u_dev, fh_assemble_vector_dev and torch element-wise updates
on u, prev, f and the lumped mass.  One process, one GPU, Hex8 Laplace and LinearElastic, the face x = 0 held, a body load, one stage
(forward Euler) and eight, dt = 0.5 (s^2 + s) / omega_max^2 of fh_dynamics_stable_dt.  Every config is measured `runs` times; one JSON
line per measurement, printed and appended to profiles/first_order.jsonl.

    python scripts/bench_first_order.py [laplace | elastic | all] [cells = 128] [steps = 200] [runs = 2]
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

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "first_order.jsonl")
RHO = 1000.0


def composed_steps(eng, u, f, m, free, dt, stages, steps):
    """the stages with the residual of fh_assemble_vector_dev: what a caller wrote before fh_first_order_create"""
    r = torch.empty_like(u)
    w1dt = 2.0 / (stages * stages + stages) * dt
    for _ in range(steps):
        prev = u
        for k in range(1, stages + 1):
            eng.set_u(u)
            r.zero_()
            eng.assemble_vector(r)
            w = (f - r) / m * free
            if k == 1:
                y = u + w1dt * w
            else:
                mu, nu = (2.0 * k - 1.0) / k, (1.0 - k) / k
                y = mu * u + nu * prev + (mu * w1dt) * w
            prev, u = u, y
    return u


def measure(label, cells, operator, scalar, stages, steps):
    mesh = fa.procedural.create_unit_box_uniform_hex_mesh_3d(cells)
    w, p = quadrature.tensor.hexahedron_gauss(2)
    qt = fa.UniformQuadratureTable.from_points_and_weights(p, w)
    if not scalar:
        qt = qt.with_uniform_data(fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.2)))
    eng = fa.Engine(0, stream=torch.cuda.current_stream().cuda_stream)
    S = 1 if scalar else 3
    n = S * mesh.num_nodes()
    bc = np.where(mesh.vertices[:, 0] < 1e-9)[0]
    asm = (fa.ElementEllipticAssemblerBuilder(eng).with_finite_element_space(mesh).with_operator(operator).with_quadrature_table(qt)
           .with_u(np.zeros(n)).build())
    f = torch.zeros(n, dtype=torch.float64, device="cuda")
    f[0::S] = (1.0 if scalar else 2.0e4) / mesh.num_nodes()
    zero = torch.zeros(n, dtype=torch.float64, device="cuda")
    out = {"config": label, "elements": mesh.num_elements(), "nodes": mesh.num_nodes(), "stages": stages, "steps": steps}
    ti = fa.RungeKuttaLegendre(asm, RHO, 1.0, stages=stages).with_dirichlet_nodes(bc)
    ti.set_state(zero)
    dt = 0.5 * ti.stable_dt(30)[1]
    out["dt"] = dt
    ti.close()
    ti = fa.RungeKuttaLegendre(asm, RHO, dt, stages=stages).with_dirichlet_nodes(bc).with_load(f)
    ti.set_state(zero)
    ti.step(20)   # warm-up: tiles, lumped mass, the check of the state
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rec = ti.step(steps)
    torch.cuda.synchronize()
    out["fused_stages_per_s"] = steps * stages / (time.perf_counter() - t0)
    out["fused_ms_per_stage"] = 1e3 / out["fused_stages_per_s"]
    out["mass_norm_end"] = float(rec.mass_norm[-1])
    u_f = ti.state(device=True)[0].clone()
    ti.close()
    # the composed stages, from the same initial state, for the same number of steps in all (so the two ends can be compared)
    m = fa.MatrixFreeMass(asm, RHO).lumped(device=True)
    free = torch.ones(n, dtype=torch.float64, device="cuda")
    for k in range(S):
        free[S * torch.from_numpy(bc).cuda() + k] = 0.0
    u = composed_steps(eng, zero.clone(), f, m, free, dt, stages, 20)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    u = composed_steps(eng, u, f, m, free, dt, stages, steps)
    torch.cuda.synchronize()
    out["composed_stages_per_s"] = steps * stages / (time.perf_counter() - t0)
    out["composed_ms_per_stage"] = 1e3 / out["composed_stages_per_s"]
    out["fused_over_composed"] = out["fused_stages_per_s"] / out["composed_stages_per_s"]
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
    runs = int(sys.argv[4]) if len(sys.argv) > 4 else 2
    configs = []
    if which in ("laplace", "all"):
        configs.append(("Laplace", fa.LaplaceOperator(), True))
    if which in ("elastic", "all"):
        configs.append(("LinearElastic", fa.MaterialEllipticOperator(fa.LinearElasticMaterial()), False))
    for name, operator, scalar in configs:
        for stages in (1, 8):
            for _ in range(runs):
                measure(f"Hex8 {name} {cells}^3, Runge-Kutta-Legendre s = {stages}, x = 0 held", cells, operator, scalar, stages,
                        max(1, steps // stages))


if __name__ == "__main__":
    main()
