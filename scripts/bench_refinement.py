#!/usr/bin/env python3
"""Uniform refinement on the device (fh_refine_uniform + fh_set_mesh_from_refinement) against the host pair it replaces
(fh_refine_hex8_uniform + fh_set_mesh), Hex8 64^3 -> 128^3, and the device refinement of the C3 tetrahedra one level coarser (BCC 38 ->
76).  One JSON line per case, printed and appended to profiles/refinement.jsonl.  The kernels by name come from a kernel trace of the
same command:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o refine -- python scripts/bench_refinement.py

    python scripts/bench_refinement.py [hex_cells] [tet_cells]        defaults: 64 38
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fenris_amd as fa  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "refinement.jsonl")


def timed(fn, reps):
    fn()   # (warm-up: first allocations, code objects)
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(ts)), float(min(ts))


def device_pair(coarse, fine_eng, mesh):
    """(refine, set the fine engine's mesh from it) in ms, each median and minimum; the sizes"""
    coarse.set_mesh(mesh)
    sizes = coarse.refine_uniformly()
    t_refine = timed(coarse.refine_uniformly, 5)
    t_set = timed(lambda: fine_eng.set_mesh_from_refinement(coarse), 5)
    return t_refine, t_set, sizes


def emit(rec):
    line = json.dumps(rec)
    print(line)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def main():
    hex_cells = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    tet_cells = int(sys.argv[2]) if len(sys.argv) > 2 else 38
    coarse, fine_eng = fa.Engine(0), fa.Engine(0)
    mesh = fa.procedural.create_unit_box_uniform_hex_mesh_3d(hex_cells)
    t_refine, t_set, sizes = device_pair(coarse, fine_eng, mesh)
    held = {}

    def host_refine():
        held["fine"] = fa.refine_uniformly(mesh)

    h_refine = timed(host_refine, 1)
    h_set = timed(lambda: fine_eng.set_mesh(held["fine"]), 3)
    emit({"case": f"Hex8 {hex_cells}^3 -> {2 * hex_cells}^3", "fine_vertices": sizes[0], "fine_cells": sizes[1], "transfer_nnz": sizes[2],
          "device_refine_ms": t_refine[0], "device_refine_min_ms": t_refine[1], "device_set_mesh_ms": t_set[0], "device_set_mesh_min_ms": t_set[1],
          "host_refine_ms": h_refine[0], "host_set_mesh_ms": h_set[0],
          "speedup_pair": (h_refine[0] + h_set[0]) / (t_refine[0] + t_set[0])})
    tets = fa.procedural.create_unit_box_uniform_tet_mesh_3d(tet_cells)
    t_refine, t_set, sizes = device_pair(coarse, fine_eng, tets)
    emit({"case": f"Tet4 BCC {tet_cells} -> {2 * tet_cells}", "coarse_cells": tets.num_elements(), "fine_vertices": sizes[0], "fine_cells": sizes[1],
          "transfer_nnz": sizes[2], "device_refine_ms": t_refine[0], "device_refine_min_ms": t_refine[1], "device_set_mesh_ms": t_set[0],
          "device_set_mesh_min_ms": t_set[1]})
    coarse.close()
    fine_eng.close()


if __name__ == "__main__":
    main()
