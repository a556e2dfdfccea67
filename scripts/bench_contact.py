#!/usr/bin/env python3
"""What the penalty contact term (fh_set_obstacles) costs: the central-difference step (fh_dynamics_step) and the tangent's map
(fh_apply_tangent_dev) on Hex8 StableNeoHookean, a free cube of cells^3 elements shifted down by 0.01, in four variants:

    parent    another build of the library without the feature (--parent-lib PATH; left out when not given)
    none      this build, no obstacles
    floor     this build, the half-space z >= -0.005: the bottom layer of nodes, 1 / (cells + 1) of them, is inside it
    sixteen   this build, that floor and 15 balls far away: FH_MAX_OBSTACLES obstacles evaluated at every node
    floor_mu0   this build, that floor with fh_set_friction given mu = 0 (the friction flag stays clear: the cost must be `floor`'s)
    floor_mu05  this build, that floor with mu = 0.5, slip velocity 0.05: the friction term in the step's node pass and in the map
    floor_mu05_moving  (--moving) `floor_mu05` with the floor sliding sideways along a path at 0.5 under nodes that start at rest: the integrator moves the
                contact clock before every launch and the node pass takes the slip relative to the floor; held against `floor_mu05`
    parent_floor  the parent's library on the `floor` scene (friction never set there: what `floor` and `floor_mu0` are held against)

The variants alternate: every measurement is a fresh child process (one library per process), `--repeats` rounds after one discarded
warm-up round, so drift of the machine hits every variant alike.  Per variant the median and the spread (min .. max) over the rounds, one
JSON line, printed and appended to profiles/contact.jsonl.

    python scripts/bench_contact.py [--cells 64] [--steps 200] [--applies 100] [--repeats 5] [--parent-lib PATH] [--variants a,b,...] [--moving]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "contact.jsonl")
RHO = 1000.0


def child(variant, cells, steps, applies):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import fenris_amd as fa
    from fenris_amd import quadrature

    mesh = fa.procedural.create_unit_box_uniform_hex_mesh_3d(cells)
    lame = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.3)).for_stable_neo_hookean(3)
    w, p = quadrature.tensor.hexahedron_gauss(2)
    qt = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(lame)
    eng = fa.Engine(0, stream=torch.cuda.current_stream().cuda_stream)
    n = 3 * mesh.num_nodes()
    asm = (fa.ElementEllipticAssemblerBuilder(eng).with_finite_element_space(mesh)
           .with_operator(fa.MaterialEllipticOperator(fa.StableNeoHookeanMaterial())).with_quadrature_table(qt).with_u(np.zeros(n)).build())
    obstacles = None
    if variant in ("floor", "sixteen", "floor_mu0", "floor_mu05", "floor_mu05_moving"):
        k = 1e6 / cells
        if variant == "floor_mu05_moving":
            items = [fa.HalfSpace((0.0, 0.0, -0.005), (0.0, 0.0, 1.0), k, friction=0.5, path=fa.ObstaclePath.constant_velocity((0.5, 0.0, 0.0), 1.0))]
        elif variant == "floor_mu05":
            items = [fa.HalfSpace((0.0, 0.0, -0.005), (0.0, 0.0, 1.0), k, friction=0.5)]
        else:
            items = [fa.HalfSpace((0.0, 0.0, -0.005), (0.0, 0.0, 1.0), k)]
        if variant == "sixteen":
            items += [fa.Ball((10.0 + j, 10.0, 10.0), 0.5, k) for j in range(15)]
        obstacles = fa.Obstacles(items, slip_length=1e-3, slip_velocity=0.05) if variant.startswith("floor_mu05") else fa.Obstacles(items)
    u0 = torch.zeros(n, dtype=torch.float64, device="cuda")
    u0[2::3] = -0.01
    v0 = torch.zeros_like(u0)
    if variant.startswith("floor_mu"):
        v0[0::3] = 1.0     # sliding: the friction force is at its cap on every touching node

    def arm():   # mu = 0 through the C ABI (the Python layer sends fh_set_friction only for a positive coefficient)
        if variant == "floor_mu0":
            import ctypes as C

            eng._check(eng._lib.fh_set_friction(eng._h, (C.c_double * 1)(0.0), 1, 1e-3))
    ti = fa.CentralDifference(asm, RHO, 1.0)
    if obstacles is not None:
        ti.with_obstacles(obstacles)
    ti.set_state(u0)
    dt = 0.25 * ti.stable_dt(30)[1]
    ti.close()
    ti = fa.CentralDifference(asm, RHO, dt)
    if obstacles is not None:
        ti.with_obstacles(obstacles)
    ti.set_state(u0, v0)
    arm()
    ti.step(20)   # warm-up: tiles, lumped mass, a_0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rec = ti.step(steps)
    torch.cuda.synchronize()
    step_ms = 1e3 * (time.perf_counter() - t0) / steps
    ti.close()
    # the tangent's map at the shifted state
    asm.with_u(u0.cpu().numpy())
    t = fa.MatrixFreeTangent(asm)
    if obstacles is not None:
        t.with_obstacles(obstacles)
    if variant.startswith("floor_mu05"):
        t.with_friction_reference(u0)     # the lag state: the shifted u
    if variant == "floor_mu05_moving":
        eng.set_obstacle_time(0.02, 0.01)
    arm()
    x = torch.rand(n, dtype=torch.float64, device="cuda")
    y = torch.empty_like(x)
    for _ in range(10):
        t.apply(y, x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(applies):
        t.apply(y, x)
    torch.cuda.synchronize()
    apply_ms = 1e3 * (time.perf_counter() - t0) / applies
    kernel_apply = eng.last_kernel_name()
    touching = 0
    if obstacles is not None:
        touching = int((fa.Contact(eng).gap(device=True) < 0).sum().item())
    print(json.dumps({"variant": variant, "step_ms": step_ms, "apply_ms": apply_ms, "dt": dt, "stored_end": float(rec.stored[-1]),
                      "nodes": mesh.num_nodes(), "touching": touching, "kernel": kernel_apply, "y_norm": float(y.norm().item())}), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--applies", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--variants", default=None, help="comma-separated subset of the variants, in the order they alternate")
    ap.add_argument("--moving", action="store_true", help="add the floor_mu05_moving variant")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        child(a.child, a.cells, a.steps, a.applies)
        return
    variants = (["parent", "parent_floor"] if a.parent_lib else []) + ["none", "floor", "sixteen", "floor_mu0", "floor_mu05"] + (["floor_mu05_moving"] if a.moving else [])
    if a.variants:
        variants = [v for v in a.variants.split(",") if v in variants]
    rows = {v: [] for v in variants}
    for rnd in range(a.repeats + 1):
        for v in variants:
            env = dict(os.environ)
            env.pop("FENRIS_HIP_LIB", None)
            if v.startswith("parent"):
                env["FENRIS_HIP_LIB"] = os.path.abspath(a.parent_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", {"parent": "none", "parent_floor": "floor"}.get(v, v), "--cells", str(a.cells), "--steps", str(a.steps),
                   "--applies", str(a.applies)]
            out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=600).stdout.strip().splitlines()[-1]
            if rnd > 0:   # (round 0 warms the machine up)
                rows[v].append(json.loads(out))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    for v in variants:
        line = {"config": f"Hex8 StableNeoHookean {a.cells}^3", "variant": v, "rounds": a.repeats, "nodes": rows[v][0]["nodes"],
                "touching": rows[v][0]["touching"], "kernel_apply": rows[v][0]["kernel"]}
        for key in ("step_ms", "apply_ms"):
            xs = [r[key] for r in rows[v]]
            line[key] = {"median": statistics.median(xs), "min": min(xs), "max": max(xs)}
        print(json.dumps(line), flush=True)
        with open(OUT, "a") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
