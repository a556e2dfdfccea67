#!/usr/bin/env python3
"""Rayleigh-damped central-difference steps per second on the device (CentralDifference.with_damping: k_damped_pass_tiled and the one node
pass) against its two yardsticks: the undamped step of the same build, which is the floor, and the damped step composed from the public
calls that existed before it -- fh_assemble_vector_dev, fh_apply_tangent_dev and torch element-wise updates.  One process, one GPU, Hex8
LinearElastic and NeoHookean, the face x = 0 clamped, a body load along +x, dt = 0.5 dt_crit of fh_dynamics_stable_dt with the damping set,
eta_m dt = 0.1 and eta_k = 0.2 dt.  One JSON line per config, printed and appended to profiles/damping.jsonl.

    python scripts/bench_damping.py [hex8_le | hex8_nh | all] [cells = 128] [steps = 200]
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

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "damping.jsonl")
RHO = 1000.0


def composed_steps(eng, tangent, u, v, a, f, m, free, dt, eta_m, eta_k, steps):
    """the damped velocity-Verlet step from fh_assemble_vector_dev, fh_apply_tangent_dev and torch"""
    r, t = torch.empty_like(u), torch.empty_like(u)
    for _ in range(steps):
        v = v + 0.5 * dt * a
        u = u + dt * v * free
        eng.set_u(u)
        r.zero_()
        eng.assemble_vector(r)
        tangent.apply(t, v)
        a = ((f - r - eta_k * t) / m - eta_m * v) / (1.0 + 0.5 * eta_m * dt) * free
        v = v + 0.5 * dt * a
    return u, v, a


def timed(ti, n, steps):
    ti.set_state(torch.zeros(n, dtype=torch.float64, device="cuda"))
    ti.step(20)   # warm-up: tiles, lumped mass, a_0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rec = ti.step(steps)
    torch.cuda.synchronize()
    return steps / (time.perf_counter() - t0), rec


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
    omega, dt0 = ti.stable_dt(30)
    eta_k = 0.2 * 0.5 * dt0
    ti.with_damping(0.0, eta_k)
    dt = 0.5 * ti.stable_dt(30)[1]
    eta_m = 0.1 / dt
    ti.close()
    out.update(dt=dt, eta_m=eta_m, eta_k=eta_k, omega_max=omega)
    for key, damping in (("undamped", None), ("mass_only", (eta_m, 0.0)), ("damped", (eta_m, eta_k))):
        ti = fa.CentralDifference(asm, RHO, dt).with_dirichlet_nodes(bc).with_load(f)
        if damping:
            ti.with_damping(*damping)
        rate, rec = timed(ti, n, steps)
        out[key + "_steps_per_s"] = rate
        out[key + "_ms_per_step"] = 1e3 / rate
        if key == "damped":
            out["kinetic_end"] = float(rec.kinetic[-1])
            u_f = ti.state(device=True)[0].clone()
        ti.close()
    out["damped_over_undamped_time"] = out["damped_ms_per_step"] / out["undamped_ms_per_step"]
    # the composed damped step, from the same initial state, for the same number of steps in all (so the two ends can be compared)
    m = fa.MatrixFreeMass(asm, RHO).lumped(device=True)
    tangent = fa.MatrixFreeTangent(asm).with_dirichlet_nodes(bc)
    free = torch.ones(n, dtype=torch.float64, device="cuda")
    for k in range(3):
        free[3 * torch.from_numpy(bc).cuda() + k] = 0.0
    u = torch.zeros(n, dtype=torch.float64, device="cuda")
    v = torch.zeros_like(u)
    eng.set_u(u)
    r = torch.zeros_like(u)
    eng.assemble_vector(r)
    a = (f - r) / m * free
    u, v, a = composed_steps(eng, tangent, u, v, a, f, m, free, dt, eta_m, eta_k, 20)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    u, v, a = composed_steps(eng, tangent, u, v, a, f, m, free, dt, eta_m, eta_k, steps)
    torch.cuda.synchronize()
    out["composed_steps_per_s"] = steps / (time.perf_counter() - t0)
    out["composed_ms_per_step"] = 1e3 / out["composed_steps_per_s"]
    out["damped_over_composed"] = out["damped_steps_per_s"] / out["composed_steps_per_s"]
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
        measure(f"Hex8 LinearElastic {cells}^3, damped central differences, x = 0 clamped", cells, fa.LinearElasticMaterial(), steps)
    if which in ("hex8_nh", "all"):
        measure(f"Hex8 NeoHookean {cells}^3, damped central differences, x = 0 clamped", cells, fa.NeoHookeanMaterial(), steps)


if __name__ == "__main__":
    main()
