#!/usr/bin/env python
"""Point location and interpolation on the device: index build, locate and the two apply kernels for 1 M seeded
points in the unit box against create_unit_box_uniform_tet_mesh_3d(56), hipEvent times (median of 20 after 3 warm-ups) beside the bytes
each kernel must move and the device's copy rate, and the 593-tet sphere beside the numpy brute force of tests/interpolation_reference.py.
Run from the repository root; prints one JSON line."""
import json, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import fenris_amd as fa
from fenris_amd.interpolate import FixedInterpolator, SpatiallyIndexed, ValuesOrGradients

def timed(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))

out = {}
eng = fa.Engine(0)
mesh = fa.procedural.create_unit_box_uniform_tet_mesh_3d(56)
E, N = mesh.num_elements(), mesh.num_nodes()
indexed = SpatiallyIndexed.from_space(mesh, eng)
out["elements"], out["nodes"] = E, N
out["index_build_ms"] = timed(lambda: eng._check(eng._lib.fh_point_index_build(eng._h)))
g = torch.Generator(device="cuda"); g.manual_seed(1)
m = 1_000_000
pts = torch.rand((m, 3), dtype=torch.float64, device="cuda", generator=g)
out["locate_ms"] = timed(lambda: indexed.locate(pts))
elem, xi, ins = indexed.locate(pts); torch.cuda.synchronize()
out["located_inside"] = int(ins.sum().item())
fixed = FixedInterpolator.from_space_and_points(indexed, pts, ValuesOrGradients.Both)
out["interpolator_build_ms_incl_locate"] = timed(lambda: FixedInterpolator.from_space_and_points(indexed, pts, ValuesOrGradients.Both).close(), reps=5, warm=1)
for s in (1, 3):
    u = torch.rand(N * s, dtype=torch.float64, device="cuda", generator=g)
    out[f"apply_values_s{s}_ms"] = timed(lambda: fixed.interpolate(u, s))
    out[f"apply_gradients_s{s}_ms"] = timed(lambda: fixed.interpolate_gradients(u, s))
# device copy rate
a = torch.empty(1 << 27, dtype=torch.float64, device="cuda"); b = torch.empty_like(a)
ms = timed(lambda: b.copy_(a))
out["copy_GBps"] = 2 * a.numel() * 8 / ms / 1e6
# bytes each kernel must move (4 nodes per point): indices 8, values 8, gradients 24 per entry; outputs; gathers not counted
out["apply_values_s1_min_bytes"] = m * (4 * 16 + 16 + 8)
out["apply_gradients_s1_min_bytes"] = m * (4 * 32 + 16 + 24)
out["locate_min_bytes"] = m * (24 + 8 + 24 + 1)
# the sphere beside the numpy brute force
import interpolation_reference as ir
sph = fa.io.load_msh_from_file(os.path.join("tests", "golden", "msh", "sphere_tet4_593.msh"), fa.TET4)
rng = np.random.default_rng(2)
p = rng.uniform(sph.vertices.min(0), sph.vertices.max(0), (301, 3))
t0 = time.perf_counter(); ir.locate(sph.vertices, sph.connectivity, p); out["sphere_numpy_brute_force_301_points_ms"] = 1e3 * (time.perf_counter() - t0)
isph = SpatiallyIndexed.from_space(sph, eng)
pd = torch.tensor(p, device="cuda")
out["sphere_device_locate_301_points_ms"] = timed(lambda: isph.locate(pd))
print(json.dumps(out))
