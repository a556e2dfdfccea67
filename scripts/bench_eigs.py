#!/usr/bin/env python3
"""Where an LOBPCG iteration spends its time (fh_eigs_lowest_dev): Hex8 LinearElastic on cells^3 elements, one face clamped, Jacobi,
10 iterations, m = 8 and m = 32.  One JSON line per m, printed and appended to profiles/eigs.jsonl.

Two measurements per m, each after a warm-up solve of two iterations (first allocations, code objects, the tile tables of the maps):
  - the solver's own split (FENRIS_HIP_EIGS_PROFILE, fh_eigs_profile): it waits for the device after every phase and adds the host's
    wall clock to the phase -- map applications, preconditioning, Gram matrices, recombinations, residuals, dense host work.  The totals
    cover the whole solve: the opening and the closing Rayleigh-Ritz step on X alone (2 m applications each) and the iterations between;
    per_iteration divides them by the iteration count all the same, so it overstates an iteration by those two steps;
  - k_block_gram and k_block_combine on their own through fh_block_gram_dev / fh_block_combine_dev at the shapes of a full basis
    (p = q = 3 m; p = 3 m with 2 m output columns), median of `reps` calls by the host's wall clock around the call (it ends in a stream
    synchronise; the copies of the small matrices are inside), and the rate from their algorithmic bytes 8 n (p + q) and
    8 n (p + outputs q).

    python scripts/bench_eigs.py [cells] [reps] [iterations]        defaults: 128 5 10
"""
import json
import os
import sys
import time

os.environ.setdefault("FENRIS_HIP_EIGS_PROFILE", "1")   # (read by fh_create)

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fenris_amd as fa  # noqa: E402
from fenris_amd import quadrature  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "eigs.jsonl")
PHASES = ("maps", "preconditioning", "gram", "combine", "residual", "dense_host", "other", "total")


def wall_median(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(min(ts))


def solve(solver, m, iters):
    try:
        return solver.solve(m, tol=1e-12, max_iter=iters, preconditioner=fa.PRECOND_JACOBI, device=True)
    except fa.EigenSolveError as e:   # (10 iterations do not converge at this size: the partial result is what is timed)
        return e.result


def main():
    cells = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    iters = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    mesh = fa.procedural.create_unit_box_uniform_hex_mesh_3d(cells)
    w, p = quadrature.tensor.hexahedron_gauss(2)
    lame = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.3))
    qt = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(lame)
    n = 3 * mesh.num_nodes()
    eng = fa.Engine(0)
    try:
        asm = (fa.ElementEllipticAssemblerBuilder(eng).with_finite_element_space(mesh)
               .with_operator(fa.MaterialEllipticOperator(fa.LinearElasticMaterial())).with_quadrature_table(qt).with_u(np.zeros(n)).build())
        clamp = np.where(mesh.vertices[:, 2] == mesh.vertices[:, 2].min())[0].astype(np.uint64)
        solver = fa.MatrixFreeEigensolver(asm, 1000.0).with_dirichlet_nodes(clamp)
        for m in (8, 32):
            solve(solver, m, 2)
            res = solve(solver, m, iters)
            prof = solver.profile()
            del res.vectors
            torch.cuda.empty_cache()
            its = max(res.iterations, 1)
            rec = {"case": f"Hex8 {cells}^3 LinearElastic, one face clamped, Jacobi", "dofs": n, "m": m, "iterations": res.iterations,
                   "applications": res.applications, "preconditionings": res.preconditionings, "restarts": res.restarts,
                   "seconds": {k: float(v) for k, v in zip(PHASES, prof)},
                   "per_iteration_ms": {k: 1e3 * float(v) / its for k, v in zip(PHASES, prof)},
                   "ms_per_application": 1e3 * float(prof[0]) / max(res.applications, 1)}
            block = float(prof[2] + prof[3] + prof[4])
            rec["block_share_of_maps"] = block / float(prof[0]) if prof[0] > 0 else None
            # the block kernels on their own at the shapes of a full basis
            pp = 3 * m
            s_t = torch.randn((pp, n), dtype=torch.float64, device="cuda")
            t_t = torch.randn((pp, n), dtype=torch.float64, device="cuda")
            g_med, g_min = wall_median(lambda: eng.block_gram(n, pp, s_t, n, pp, t_t, n), reps)
            q = 2 * m
            c = np.random.default_rng(0).standard_normal((pp, q))
            y_t = t_t[:q]
            c_med, c_min = wall_median(lambda: eng.block_combine(n, pp, s_t, n, c, y_t, n), reps)
            gb, cb = 8 * n * (pp + pp), 8 * n * (pp + q)
            rec["k_block_gram"] = {"p": pp, "q": pp, "ms_median": 1e3 * g_med, "ms_min": 1e3 * g_min, "bytes": gb, "TB_per_s": gb / g_med / 1e12,
                                   "Tflop_per_s": 2.0 * n * pp * pp / g_med / 1e12}
            rec["k_block_combine"] = {"p": pp, "q_total": q, "ms_median": 1e3 * c_med, "ms_min": 1e3 * c_min, "bytes": cb, "TB_per_s": cb / c_med / 1e12,
                                      "Tflop_per_s": 2.0 * n * pp * q / c_med / 1e12}
            del s_t, t_t, y_t
            torch.cuda.empty_cache()
            line = json.dumps(rec)
            print(line, flush=True)
            with open(OUT, "a") as f:
                f.write(line + "\n")
    finally:
        eng.close()


if __name__ == "__main__":
    main()
