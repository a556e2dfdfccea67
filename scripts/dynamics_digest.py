#!/usr/bin/env python3
"""One SHA-256 per case over every bit the time integrators hand back: u, v, a of the state, all record rows, steps_done and stats.

A refactor of the integrators must leave every line as it is: run this on a build of the parent and on the new build (FENRIS_HIP_LIB picks
another library) and diff the two outputs.  The existing tests compare a build with itself or with the reference to a tolerance and cannot
see a bit that moved between two builds.

Every run: 7 steps cut into calls of 3 and 4 with record_every=2, on Hex8 2x2x2, Tet4 of a 2x2x2 box or Quad4 3x3 with the face x = 0
clamped.  The explicit schemes run once on the tiles and once off them (a rule-set table), and the route is checked by the kernel name.

    python scripts/dynamics_digest.py [substring of the case names to run]
"""
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fenris_amd as fa  # noqa: E402
from fenris_amd import quadrature  # noqa: E402

LAME = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.3))
RHO = 1000.0
EXPLICIT = ("central", "rkl1", "rkl3")
SECOND_ORDER = ("central", "newmark", "euler")


def mesh_of(kind):
    P, T, Q = fa.procedural, quadrature.tensor, quadrature.total_order
    if kind == "hex8":
        return P.create_unit_box_uniform_hex_mesh_3d(2), T.hexahedron_gauss(2), T.hexahedron_gauss(3)
    if kind == "tet4":
        return P.create_unit_box_uniform_tet_mesh_3d(2), Q.tetrahedron(2), Q.tetrahedron(4)
    return P.create_unit_square_uniform_quad_mesh_2d(3), T.quadrilateral_gauss(2), T.quadrilateral_gauss(3)


def operator_of(op):
    return {"laplace": fa.LaplaceOperator(), "elastic": fa.MaterialEllipticOperator(fa.LinearElasticMaterial()),
            "neo": fa.MaterialEllipticOperator(fa.NeoHookeanMaterial())}[op]


class Case:
    """one engine, one assembler, one integrator; `h` hashes everything the case hands back"""

    def __init__(self, kind, op, scheme, tiles=True, load=False, dt=None, newton=None):
        self.kind, self.op, self.scheme, self.tiles = kind, op, scheme, tiles
        m, (w, p), (w2, p2) = mesh_of(kind)
        w, p, w2, p2 = (np.asarray(a) for a in (w, p, w2, p2))
        self.mesh = m
        self.S = 1 if op == "laplace" else m.vertices.shape[1]
        self.n = self.S * m.num_nodes()
        if tiles:
            qt = fa.UniformQuadratureTable.from_points_and_weights(p, w)
            qt = qt if op == "laplace" else qt.with_uniform_data(LAME)
        else:   # two rules, alternating over the elements: the residual is summed rule by rule
            emap = (np.arange(len(m.connectivity)) % 2).astype(np.uint64)
            data = None if op == "laplace" else [[LAME] * len(w), [LAME] * len(w2)]
            qt = fa.compact_quadrature_table([p, p2], [w, w2], data, emap)
        self.eng = fa.Engine(0)
        self.asm = (fa.ElementEllipticAssemblerBuilder(self.eng).with_finite_element_space(m).with_operator(operator_of(op))
                    .with_quadrature_table(qt).with_u(np.zeros(self.n)).build())
        first = scheme not in SECOND_ORDER
        dt = dt if dt is not None else (1e-5 if first and op != "laplace" else 1e-3)
        if scheme == "central":
            ti = fa.CentralDifference(self.asm, RHO, dt)
        elif scheme in ("newmark", "euler"):
            ti = (fa.Newmark if scheme == "newmark" else fa.BackwardEuler)(self.asm, RHO, dt)
        elif scheme.startswith("rkl"):
            ti = fa.RungeKuttaLegendre(self.asm, RHO, dt, stages=int(scheme[3:]))
        else:
            ti = fa.ThetaMethod(self.asm, RHO, dt, theta=float(scheme[5:]))
        if scheme not in EXPLICIT:
            ti.with_newton(fa.NewtonSettings(*(newton or (40, 1e-10))), linear_rel_tol=1e-12)
        x = m.vertices[:, 0]
        self.clamp = np.where(np.isclose(x, x.min()))[0]
        ti.with_dirichlet_nodes(self.clamp)
        if load:
            ti.with_load(self.force(1.0), np.linspace(0.25, 1.0, 5))
        self.ti = ti
        self.first = first
        self.h = hashlib.sha256()
        i = np.arange(self.n)
        self.u0, self.v0 = 0.01 * np.sin(i + 1.0), 0.05 * np.cos(0.5 * i)

    def force(self, scale):
        return scale * (200.0 if self.op != "laplace" else 1.0) * np.cos(0.3 * np.arange(self.n))

    def start(self):
        self.ti.set_state(self.u0, None if self.first else self.v0)
        return self

    def eat(self, *arrays):
        for a in arrays:
            self.h.update(np.ascontiguousarray(a).tobytes())

    def eat_state(self):
        u, v, a, t, k = fa.TimeIntegrator.state(self.ti)   # (first order: the rate is v)
        self.eat(u, v, a, np.float64(t), np.uint64(k))

    def check_route(self):
        """after a state() that has just formed a_0 (the rate): the route of the scheme's own launch"""
        name = self.eng.last_kernel_name()
        if self.scheme in EXPLICIT and name.endswith("_from_partials") != self.tiles:
            raise RuntimeError(f"the case was to run {'on' if self.tiles else 'off'} the tiles and ran {name}")

    def eat_record(self, rec):
        self.eat(rec.kinetic, rec.stored, rec.load_potential, rec.time, np.uint64(rec.steps_done), np.asarray(rec.stats, dtype=np.uint64))

    def step(self, n, every=2):
        try:
            self.eat_record(self.ti.step(n, record_every=every))
        except fa.FenrisError as err:   # a failed step is part of what a build computes: its code, its record and the state left behind
            self.eat(np.int64(err.code), np.uint64(getattr(err, "steps_done", 0)))
            if hasattr(err, "record"):
                self.eat_record(err.record)
            return False
        return True

    def run(self):
        """state (a_0), 3 steps, 4 steps, state"""
        self.eat_state()
        self.check_route()
        self.step(3)
        self.step(4)
        self.eat_state()
        return self.close()

    def close(self):
        self.ti.close()
        self.eng.close()
        return self.h.hexdigest()


def floor(friction, path):
    p = fa.ObstaclePath.constant_velocity((0.5, 0.0, 0.0), 1.0) if path else None
    return fa.Obstacles([fa.HalfSpace((0.0, 0.0, 0.02), (0.0, 0.0, 1.0), 1e5, friction=friction, path=p)], slip_length=1e-3,
                        slip_velocity=0.05) if friction else fa.Obstacles([fa.HalfSpace((0.0, 0.0, 0.02), (0.0, 0.0, 1.0), 1e5, path=p)])


def cases():
    out = {}
    routes = lambda scheme: (True, False) if scheme in EXPLICIT else (True,)   # noqa: E731
    # every scheme on every mesh and operator, with and without a load and a load-factor table
    for kind, op in (("hex8", "elastic"), ("hex8", "neo"), ("tet4", "neo"), ("quad4", "elastic"), ("quad4", "laplace")):
        for scheme in ("central", "newmark", "euler", "rkl1", "rkl3", "theta0.5", "theta1"):
            for load in (False, True):
                for tiles in routes(scheme):
                    name = f"{kind}-{op}-{scheme}-{'load' if load else 'free'}-{'tiles' if tiles else 'summed'}"
                    out[name] = lambda a=(kind, op, scheme, tiles, load): Case(*a).start().run()
    # Rayleigh damping, mass and stiffness: central differences, Newmark on a linear operator
    for scheme in ("central", "newmark"):
        for tiles in routes(scheme):
            def damped(scheme=scheme, tiles=tiles):
                c = Case("hex8", "elastic", scheme, tiles, load=True)
                c.ti.with_damping(2.0, 1e-4)
                return c.start().run()
            out[f"damped-{scheme}-{'tiles' if tiles else 'summed'}"] = damped
    # a plane obstacle with friction and a slip velocity; the same obstacle on a path
    for what in ("friction", "path", "friction-path"):
        for scheme in ("central", "euler"):
            for tiles in routes(scheme):
                def contact(what=what, scheme=scheme, tiles=tiles):
                    c = Case("hex8", "elastic", scheme, tiles)
                    c.ti.with_obstacles(floor(0.5 if "friction" in what else 0.0, "path" in what))
                    c.v0 = c.v0 + np.tile([1.0, 0.0, 0.0], c.n // 3)   # sliding along the floor
                    return c.start().run()
                out[f"{what}-{scheme}-{'tiles' if tiles else 'summed'}"] = contact
    # a prescribed motion of the clamped face
    for scheme in ("central", "euler"):
        for tiles in routes(scheme):
            def moved(scheme=scheme, tiles=tiles):
                c = Case("hex8", "neo", scheme, tiles)
                factor = 0.02 * np.sin(np.linspace(0.0, 1.0, 6))
                c.ti.with_boundary_motion(np.ones(c.n), factor)
                c.v0[np.repeat(c.clamp * c.S, c.S) + np.tile(np.arange(c.S), len(c.clamp))] = (factor[1] - factor[0]) / c.ti.dt
                return c.start().run()
            out[f"motion-{scheme}-{'tiles' if tiles else 'summed'}"] = moved
    # a Newton failure: one iteration where the step needs more; the digest takes the state left behind
    for scheme in ("newmark", "theta0.5"):
        def failing(scheme=scheme):
            c = Case("hex8", "neo", scheme, load=True, dt=1e-2 if scheme == "newmark" else 1e-4, newton=(1, 1e-13)).start()
            if c.step(3):
                raise RuntimeError("the Newton step was to fail and did not")
            c.eat_state()
            c.step(2)
            c.eat_state()
            return c.close()
        out[f"newton-failure-{scheme}"] = failing
    # a_n asked for before the first step, and again after the load and the damping change mid-run
    for scheme in ("central", "newmark"):
        def stale(scheme=scheme):
            c = Case("hex8", "elastic", scheme, load=True).start()
            c.eat_state()
            c.step(3)
            c.ti.with_load(c.force(-0.5), np.linspace(1.0, 2.0, 4))
            c.eat_state()
            c.step(2)
            c.ti.with_damping(1.0, 5e-5)
            c.eat_state()
            c.step(2)
            c.eat_state()
            return c.close()
        out[f"stale-a-{scheme}"] = stale
    # stable_dt: the two doubles
    for what in ("undamped", "stiffness-damped", "rkl3"):
        def stable(what=what):
            c = Case("hex8", "elastic", "rkl3" if what == "rkl3" else "central")
            if what == "stiffness-damped":
                c.ti.with_damping(0.0, 1e-4)
            c.start()
            c.eat(np.asarray(c.ti.stable_dt(5), dtype=np.float64))
            return c.close()
        out[f"stable-dt-{what}"] = stable
    return out


def main():
    pick = sys.argv[1] if len(sys.argv) > 1 else ""
    t0 = time.perf_counter()
    failed = 0
    for name, run in cases().items():
        if pick not in name:
            continue
        try:
            print(f"{name} {run()}", flush=True)
        except Exception as err:   # (a case that cannot run is no digest)
            failed += 1
            print(f"{name} FAILED {type(err).__name__}: {err}", flush=True)
    print(f"# {time.perf_counter() - t0:.1f} s", file=sys.stderr)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
