#!/usr/bin/env python3
"""What the per-element expansion (fh_set_element_expansion) costs: the residual (fh_assemble_vector_dev) and the tangent's map
(fh_apply_tangent_dev) on the tiled kinds -- Hex8 (jittered, and axis-aligned: the monomial and moment forms) and Tet4, linear elasticity and
Neo-Hookean -- in these variants:

    parent   another build of the library without the feature (--parent-lib PATH; left out when not given)
    unset    this build, no field: the instantiations the parent has
    ones     this build, a field of ones.  The host hands the kernels no field for it, so this runs the kernels of `unset` and measures
             the host's flag alone: the cost must be `unset`'s
    uniform  this build, one stretch for the mesh, 1 + 1e-9 (count == 1): the second instantiations on uniform data
    random   this build, one stretch per element, uniform in [0.95, 1.05]: the second instantiations

The variants alternate as in scripts/ab_bench.py: every measurement is a fresh child process (one library per process), `--repeats` rounds
after one discarded warm-up round, so drift of the machine hits every variant alike.  Per case and variant the median and the spread
(min .. max) over the rounds in microseconds per call and the ratio to `unset`; one JSON line, printed and appended to
profiles/element_expansion.jsonl.

    python scripts/bench_expansion.py [--cells 64] [--calls 100] [--repeats 5] [--parent-lib PATH]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "element_expansion.jsonl")
CASES = [("hex8", "elastic"), ("hex8", "neo_hookean"), ("hex8_affine", "elastic"), ("hex8_affine", "neo_hookean"), ("tet4", "elastic"),
         ("tet4", "neo_hookean")]


def child(variant, cells, calls):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import fenris_amd as fa
    from fenris_amd import quadrature

    out = {}
    rng = np.random.default_rng(0)
    for kind, op in CASES:
        if kind.startswith("hex8"):
            mesh = fa.procedural.create_unit_box_uniform_hex_mesh_3d(cells)
            if kind == "hex8":
                mesh = fa.Mesh(mesh.vertices + (0.1 / cells) * rng.uniform(-1.0, 1.0, mesh.vertices.shape), mesh.connectivity, mesh.elem_kind)
            w, p = quadrature.tensor.hexahedron_gauss(2)
        else:
            mesh = fa.procedural.create_unit_box_uniform_tet_mesh_3d(max(2, cells // 2))
            w, p = quadrature.total_order.tetrahedron(2)
        lame = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.3))
        qt = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(lame)
        eng = fa.Engine(0, stream=torch.cuda.current_stream().cuda_stream)
        n = 3 * mesh.num_nodes()
        u = 0.01 * np.sin(np.arange(n))
        material = fa.LinearElasticMaterial() if op == "elastic" else fa.NeoHookeanMaterial()
        asm = (fa.ElementEllipticAssemblerBuilder(eng).with_finite_element_space(mesh).with_operator(fa.MaterialEllipticOperator(material))
               .with_quadrature_table(qt).with_u(u).build())
        if variant == "ones":
            eng.set_element_expansion(np.ones(mesh.num_elements()))
        elif variant == "uniform":
            eng.set_element_expansion(1.0 + 1e-9)
        elif variant == "random":
            eng.set_element_expansion(rng.uniform(0.95, 1.05, mesh.num_elements()))
        x = torch.tensor(np.cos(np.arange(n)), device="cuda:0")
        y = torch.zeros(n, dtype=torch.float64, device="cuda:0")
        tangent = fa.MatrixFreeTangent(asm)
        tangent._bind()

        def timed(fn):
            for _ in range(5):
                fn()
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(calls):
                fn()
            t1.record()
            torch.cuda.synchronize()
            return 1e3 * t0.elapsed_time(t1) / calls   # microseconds per call

        out[f"{kind}.{op}.residual"] = timed(lambda: eng.assemble_vector_async(y))
        out[f"{kind}.{op}.tangent"] = timed(lambda: eng.apply_tangent_dev(x, y))
        eng.poll_status()
        del tangent, asm
        eng.close()
    print("RESULT " + json.dumps(out))


def run_child(variant, args):
    env = dict(os.environ)
    name = variant
    if variant == "parent":
        env["FENRIS_HIP_LIB"] = args.parent_lib
        name = "unset"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--cells", str(args.cells), "--calls", str(args.calls)], env=env,
                       capture_output=True, text=True, timeout=600)
    for line in r.stdout.splitlines():
        if line.startswith("RESULT "):
            return json.loads(line[7:])
    raise RuntimeError(f"{variant}: no result\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=64)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib")
    ap.add_argument("--child")
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.cells, args.calls)
    variants = (["parent"] if args.parent_lib else []) + ["unset", "ones", "uniform", "random"]
    rounds = {v: [] for v in variants}
    for r in range(args.repeats + 1):
        for v in variants:
            res = run_child(v, args)
            if r > 0:   # (the first round warms the machine up)
                rounds[v].append(res)
    summary = {"cells": args.cells, "calls": args.calls, "repeats": args.repeats, "cases": {}}
    for key in rounds["unset"][0]:
        row = {}
        for v in variants:
            t = [r[key] for r in rounds[v]]
            row[v] = {"median_us": statistics.median(t), "min_us": min(t), "max_us": max(t)}
        base = row["unset"]["median_us"]
        for v in variants:
            row[v]["ratio_to_unset"] = row[v]["median_us"] / base
        summary["cases"][key] = row
    line = json.dumps(summary)
    print(line)
    with open(OUT, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
