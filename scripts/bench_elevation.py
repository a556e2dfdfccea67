#!/usr/bin/env python3
"""Degree elevation on the device (fh_elevate_degree) against the host sweeps it mirrors (fh_hex8_to_hex27, fh_refine_to_quadratic):
Hex8 128^3 -> Hex27 and Tet4 BCC 56 -> Tet10.  One JSON line per case, printed and appended to profiles/degree_elevation.jsonl.

The device call ends in a stream synchronise, so two clocks agree on it and both are reported: device events on the default stream around
the call, and the host's wall clock; medians over `reps` calls after a warm-up call.  The host sweep runs once, by wall clock.  The bytes
are the least the passes can move, counted from the shapes (see bytes_moved); the rate is those bytes over the device time, to set against
a copy's 6.3 TB/s.  The kernels by name come from a kernel trace of the same command:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o elevate -- python scripts/bench_elevation.py

    python scripts/bench_elevation.py [hex_cells] [tet_cells] [reps]        defaults: 128 56 7
"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fenris_amd as fa  # noqa: E402
from fenris_amd import _ffi  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "degree_elevation.jsonl")
# (labelled slots per cell, of which sorted) of the high kinds: label_table, engine_hierarchy.hip
SLOTS = {fa.HEX27: (27, 26), fa.HEX20: (20, 20), fa.TET10: (10, 10), fa.QUAD9: (5, 4), fa.TRI6: (3, 3)}


def bytes_moved(lin, to_kind, nodes, nnz):
    """least traffic of the passes in bytes: keys (read the cells, write key + id), the radix sort (8 bits per pass over 2 * bits key
    bits, key + id read and written per pass), first (read key + id, write first + val), the scan (8 in, 8 out), cells (first + scan in,
    one word out), rows (first + scan in per candidate; per node its position, offset and row out)"""
    E, nv = lin.num_elements(), lin.connectivity.shape[1]
    S, Sm = SLOTS[to_kind]
    nlab, nsort = E * S, E * Sm
    d = lin.vertices.shape[1]
    bits = max(1, int(lin.num_nodes()).bit_length())
    passes = -(-2 * bits // 8)
    parts = {
        "keys": 4 * E * nv + 12 * nsort,
        "sort": passes * 24 * nsort,
        "first": 24 * nsort,
        "scan": 16 * nlab,
        "cells": 12 * nlab + 8 * E * _ffi.ELEM_NODES[to_kind],
        "rows": 12 * nlab + nodes * (8 * d + 8) + 16 * nnz + 8 * d * lin.num_nodes(),
    }
    return parts, passes


def timed_device(fn, reps):
    fn()   # (warm-up: first allocations, code objects, the sort's tuning)
    ev, wall = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
        ev.append(a.elapsed_time(b))
    return float(np.median(ev)), float(min(ev)), float(np.median(wall))


def case(eng, name, lin, to_kind, host, reps):
    eng.set_mesh(lin)
    nodes, nnz = eng.elevate_degree(to_kind)
    ev, ev_min, wall = timed_device(lambda: eng.elevate_degree(to_kind), reps)
    t0 = time.perf_counter()
    ref = host(lin)
    host_ms = 1e3 * (time.perf_counter() - t0)
    high, _ = eng.degree_elevation()
    same = bool(np.array_equal(high.connectivity, ref.connectivity) and np.array_equal(high.vertices.view(np.uint64), ref.vertices.view(np.uint64)))
    parts, passes = bytes_moved(lin, to_kind, nodes, nnz)
    total = sum(parts.values())
    rec = {"case": name, "cells": lin.num_elements(), "linear_vertices": lin.num_nodes(), "high_nodes": nodes, "transfer_nnz": nnz,
           "device_ms_events_median": ev, "device_ms_events_min": ev_min, "device_ms_wall_median": wall, "host_ms": host_ms,
           "speedup": host_ms / ev, "bit_identical_to_host": same, "radix_passes": passes, "bytes": parts, "bytes_total": total,
           "rate_TB_per_s": total / (ev * 1e-3) / 1e12, "kernels": eng.last_kernel_name()}
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def main():
    hex_cells = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    tet_cells = int(sys.argv[2]) if len(sys.argv) > 2 else 56
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 7
    eng = fa.Engine(0)
    try:
        case(eng, f"Hex8 {hex_cells}^3 -> Hex27", fa.procedural.create_unit_box_uniform_hex_mesh_3d(hex_cells), fa.HEX27, fa.hex27_mesh_from_hex8, reps)
        case(eng, f"Tet4 BCC {tet_cells} -> Tet10", fa.procedural.create_unit_box_uniform_tet_mesh_3d(tet_cells), fa.TET10, fa.tet10_mesh_from_tet4, reps)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
