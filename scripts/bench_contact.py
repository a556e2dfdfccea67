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
    floor_aug   this build, that floor with augmented-Lagrangian multipliers standing (fh_set_contact_multipliers: the penetration of the
                bottom layer, what one update of the shifted state gives): the node pass and the map take the instantiation with the shift
                and load one multiplier per node; held against `floor`
    floor_aug_mu05  `floor_mu05` with the same multipliers standing; held against `floor_mu05`
    parent_floor  the parent's library on the `floor` scene (friction never set there: what `floor` and `floor_mu0` are held against)
    parent_sixteen  the parent's library on the `sixteen` scene
    floor_grid  this build, that floor as a sampled signed-distance grid (fh_sdf_grid_create): 17^3 samples of its linear field over
                [-0.25, 1.25]^3, which covers the cube; held against `floor`: what the 8 gathers per node and the interpolation cost
    ball        this build, a ball of radius 0.4 whose lowest point is 0.03 below the top face of the unshifted cube
    ball_grid   this build, that ball sampled at 64^3 over the same box; held against `ball`

--digest (with --parent-lib): no timing; both libraries compute the stand-alone pieces of the term (energy, gap, force, CSR blocks, the
tangent's map and diagonal, resultants, and with friction, a lag state and paths the potential, force, blocks and resultants) for a
half-space, a ball and a cavity on six small meshes, and the SHA-256 digests of the bytes are compared: a build that adds an obstacle kind
must not move a bit of the kinds that were there.  On a build with multipliers the same pieces are formed again with all-zero multipliers
standing (they must be the bytes of none: counted as moved otherwise) and with random ones (digests reported for this build alone).

The variants alternate: every measurement is a fresh child process (one library per process), `--repeats` rounds after one discarded
warm-up round, so drift of the machine hits every variant alike.  Per variant the median and the spread (min .. max) over the rounds, one
JSON line, printed and appended to profiles/contact.jsonl.

    python scripts/bench_contact.py [--cells 64] [--steps 200] [--applies 100] [--repeats 5] [--parent-lib PATH] [--variants a,b,...] [--moving]
    python scripts/bench_contact.py --digest --parent-lib PATH
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
    if variant in ("floor", "sixteen", "floor_mu0", "floor_mu05", "floor_mu05_moving", "floor_aug", "floor_aug_mu05"):
        k = 1e6 / cells
        if variant == "floor_mu05_moving":
            items = [fa.HalfSpace((0.0, 0.0, -0.005), (0.0, 0.0, 1.0), k, friction=0.5, path=fa.ObstaclePath.constant_velocity((0.5, 0.0, 0.0), 1.0))]
        elif variant in ("floor_mu05", "floor_aug_mu05"):
            items = [fa.HalfSpace((0.0, 0.0, -0.005), (0.0, 0.0, 1.0), k, friction=0.5)]
        else:
            items = [fa.HalfSpace((0.0, 0.0, -0.005), (0.0, 0.0, 1.0), k)]
        if variant == "sixteen":
            items += [fa.Ball((10.0 + j, 10.0, 10.0), 0.5, k) for j in range(15)]
        obstacles = fa.Obstacles(items, slip_length=1e-3, slip_velocity=0.05) if variant.endswith(("mu05", "mu05_moving")) else fa.Obstacles(items)
    if variant in ("floor_grid", "ball", "ball_grid"):
        k = 1e6 / cells
        centre = (0.5, 0.5, 1.0 + 0.4 - 0.03)
        if variant == "ball":
            items = [fa.Ball(centre, 0.4, k)]
        else:
            f = (lambda x: x[:, 2] + 0.005) if variant == "floor_grid" else fa.sdf_circle(centre, 0.4)
            grid, origin = fa.SdfGrid.from_function(f, (-0.25,) * 3, (1.25,) * 3, (17,) * 3 if variant == "floor_grid" else (64,) * 3)
            items = [fa.GridObstacle(grid, origin, k)]
        obstacles = fa.Obstacles(items)
    u0 = torch.zeros(n, dtype=torch.float64, device="cuda")
    u0[2::3] = -0.01
    v0 = torch.zeros_like(u0)
    if variant.startswith("floor_mu") or variant == "floor_aug_mu05":
        v0[0::3] = 1.0     # sliding: the friction force is at its cap on every touching node

    def arm():   # mu = 0 through the C ABI (the Python layer sends fh_set_friction only for a positive coefficient)
        if variant == "floor_mu0":
            import ctypes as C

            eng._check(eng._lib.fh_set_friction(eng._h, (C.c_double * 1)(0.0), 1, 1e-3))
        if variant.startswith("floor_aug"):   # the multipliers: the penetration of the bottom layer at the shifted state
            s = np.zeros((1, mesh.num_nodes()))
            s[0, np.isclose(np.asarray(mesh.vertices)[:, 2], 0.0)] = 0.005
            fa.Contact(eng).set_multipliers(s)
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
    if variant.endswith(("mu05", "mu05_moving")):
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


def digest_child():
    """one line of JSON: the SHA-256 digests of the pieces of the term for the three analytic kinds, per mesh and piece"""
    import hashlib

    import numpy as np

    sys.path.insert(0, ROOT)
    import fenris_amd as fa
    from fenris_amd import _ffi, quadrature

    P, T, Q = fa.procedural, quadrature.tensor, quadrature.total_order
    meshes = {"HEX8": (P.create_unit_box_uniform_hex_mesh_3d(2), T.hexahedron_gauss(2)), "TET4": (P.create_unit_box_uniform_tet_mesh_3d(2), Q.tetrahedron(2)),
              "QUAD4": (P.create_unit_square_uniform_quad_mesh_2d(3), T.quadrilateral_gauss(2)), "TRI3": (P.create_unit_square_uniform_tri_mesh_2d(3), Q.triangle(2)),
              "TET10": (fa.tet10_mesh_from_tet4(P.create_unit_box_uniform_tet_mesh_3d(2)), Q.tetrahedron(4)),
              "HEX8_7": (P.create_unit_box_uniform_hex_mesh_3d(7), T.hexahedron_gauss(2))}
    lame = fa.LameParameters(384.0, 577.0)
    out = {}
    eng = fa.Engine(0)
    for name, (m, (w, p)) in meshes.items():
        X = np.asarray(m.vertices)
        N, d = X.shape
        rng = np.random.default_rng(31)
        ubar = rng.uniform(-0.02, 0.02, N * d)
        u = ubar + rng.uniform(-0.02, 0.02, N * d)
        wn = rng.uniform(0.5, 2.0, N)
        x = rng.uniform(-1.0, 1.0, N * d)
        path = fa.ObstaclePath([0.0, 2.0], [[0.0] * d, [0.03125, -0.015625, 0.0078125][:d]])

        def obstacles(mu):
            return fa.Obstacles([fa.HalfSpace((0.3,) * d, (1.0, 2.0, 3.0)[:d], 1.0e4, friction=0.5 * mu, path=path), fa.Ball((1.1,) * d, 0.7, 2.0e3, friction=0.3 * mu),
                                 fa.Cavity((0.4, 0.5, 0.6)[:d], 0.75 if d == 3 else 0.6, 5.0e3, friction=0.7 * mu, path=path)], wn, slip_length=2e-3)

        qt = fa.UniformQuadratureTable.from_points_and_weights(np.asarray(p), np.asarray(w)).with_uniform_data(lame)
        asm = (fa.ElementEllipticAssemblerBuilder(eng).with_finite_element_space(m).with_operator(fa.MaterialEllipticOperator(fa.NeoHookeanMaterial()))
               .with_quadrature_table(qt).with_u(u).build())
        pieces = {}
        has_multipliers = hasattr(eng._lib, "fh_set_contact_multipliers")
        s_random = rng.uniform(0.0, 0.05, (3, N)) * rng.choice([0.0, 1.0, 20.0], (3, N))
        modes = [("", None)] + ([(" zero", np.zeros((3, N))), (" aug", s_random)] if has_multipliers else [])
        for mu, (tag, s_mult) in ((mu, mode) for mu in (0.0, 1.0) for mode in modes):
            eng.set_obstacles(obstacles(mu))
            if mu:
                eng._check(eng._lib.fh_set_friction_reference(eng._h, _ffi.fp(np.ascontiguousarray(ubar))))
            eng.set_obstacle_time(1.25, 0.75)
            con = fa.Contact(eng)
            if s_mult is not None:
                con.set_multipliers(s_mult)
            mu = f"{mu}{tag}"
            k = fa.CsrAssembler(fa.SCATTER_GATHER).assemble(asm)
            vals = np.zeros_like(k.values)
            con.add_tangent_to(vals)
            R, Qf = con.resultants()
            pieces.update({f"energy{mu}": np.array([con.energy(), con.friction_potential()]), f"gap{mu}": con.gap(), f"force{mu}": con.force(),
                           f"friction force{mu}": con.friction_force(), f"csr{mu}": vals, f"resultants{mu}": np.concatenate([R.ravel(), Qf.ravel()])})
            t = fa.MatrixFreeTangent(asm).with_obstacles(obstacles(float(mu.split()[0])))
            if float(mu.split()[0]):
                t.with_friction_reference(ubar)
            eng.set_obstacle_time(1.25, 0.75)
            if s_mult is not None:
                con.set_multipliers(s_mult)
            pieces[f"apply{mu}"] = t.apply(np.zeros(N * d), x).copy()
            pieces[f"diagonal{mu}"] = t.diagonal()
            t.with_obstacles(None)
        assert np.abs(pieces["force0.0"]).max() > 0 and np.abs(pieces["friction force1.0"]).max() > 0
        for key, a in pieces.items():
            out[f"{name} {key}"] = hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()[:16]
    eng.close()
    print(json.dumps(out), flush=True)


def digest(parent_lib):
    got = {}
    for which in ("parent", "this"):
        env = dict(os.environ)
        env.pop("FENRIS_HIP_LIB", None)
        if which == "parent":
            env["FENRIS_HIP_LIB"] = os.path.abspath(parent_lib)
        got[which] = json.loads(subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "digest"], env=env, check=True, capture_output=True,
                                               text=True, timeout=600).stdout.strip().splitlines()[-1])
    this, parent = got["this"], got["parent"]
    shared = {k: v for k, v in this.items() if k in parent}
    moved = [k for k in shared if shared[k] != parent[k]]

    def base_of(key):   # "HEX8 force0.0 zero" -> "HEX8 force0.0"
        return key[:-len(" zero")]

    moved += [k for k in this if k.endswith(" zero") and this[k] != this.get(base_of(k))]       # all-zero multipliers: the bytes of none
    aug = {k: v for k, v in this.items() if k.endswith(" aug")}
    # (random multipliers must show in the force, the map, the diagonal and the blocks)
    same = [k for k in aug if k.split()[1].startswith(("force", "apply", "csr", "diagonal")) and aug[k] == this.get(k[:-len(" aug")])]
    print(json.dumps({"digest": True, "pieces": len(shared), "moved": moved, "parent": hashlib_of(parent), "this": hashlib_of(shared),
                      "zero_multiplier_pieces": sum(k.endswith(" zero") for k in this), "multiplier_pieces": len(aug),
                      "multipliers": hashlib_of(aug), "multipliers_without_effect": same}), flush=True)
    return 1 if moved or same or len(shared) != len(parent) else 0


def hashlib_of(table):
    import hashlib

    return hashlib.sha256(json.dumps(table, sort_keys=True).encode()).hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=64)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--applies", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--variants", default=None, help="comma-separated subset of the variants, in the order they alternate")
    ap.add_argument("--moving", action="store_true", help="add the floor_mu05_moving variant")
    ap.add_argument("--digest", action="store_true", help="compare the bytes of the three analytic kinds between --parent-lib and this build")
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child == "digest":
        digest_child()
        return
    if a.child:
        child(a.child, a.cells, a.steps, a.applies)
        return
    if a.digest:
        if not a.parent_lib:
            ap.error("--digest needs --parent-lib")
        sys.exit(digest(a.parent_lib))
    variants = ((["parent", "parent_floor", "parent_sixteen"] if a.parent_lib else []) + ["none", "floor", "floor_aug", "sixteen", "floor_mu0", "floor_mu05", "floor_aug_mu05"] + (["floor_mu05_moving"] if a.moving else [])
                + ["floor_grid", "ball", "ball_grid"])
    if a.variants:
        variants = [v for v in a.variants.split(",") if v in variants]
    rows = {v: [] for v in variants}
    for rnd in range(a.repeats + 1):
        for v in variants:
            env = dict(os.environ)
            env.pop("FENRIS_HIP_LIB", None)
            if v.startswith("parent"):
                env["FENRIS_HIP_LIB"] = os.path.abspath(a.parent_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", {"parent": "none", "parent_floor": "floor", "parent_sixteen": "sixteen"}.get(v, v), "--cells", str(a.cells), "--steps", str(a.steps),
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
