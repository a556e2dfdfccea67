"""Recovered quantities of a solved field: displacement gradient, strain, stresses, energy density and element volumes at the
quadrature points, per element and at the nodes, over fh_recover* (include/fenris_hip.h).

    engine = assembler.engine                       # mesh, operator, quadrature table and u as the residual sees them
    sigma = engine.recover("cauchy_stress", "nodes")         # torch tensor on the engine's device, (N, d, d)
    rec = Recovery(engine)
    vm = rec.von_mises("elements")                            # (E,)
    x = engine.physical_quadrature_points(nq); p = rec.stress_pk1("points")     # rows pair up: (E nq, s, d)

`where` is "points" (one row per element and quadrature point, the order of fh_physical_quadrature_points), "elements" (the
measure-weighted mean over the element's points) or "nodes" (the volume-weighted average of those means over the node's active elements --
a patch average, not an L2 projection).  The 2-D von Mises stress is the in-plane form.  All numerics run in libfenris_hip.so on the GPU;
there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

from . import _ffi
from .assembly import Engine

QUANTITIES = {"grad_u": _ffi.RECOVER_GRAD_U, "strain": _ffi.RECOVER_STRAIN, "stress_pk1": _ffi.RECOVER_STRESS_PK1,
              "cauchy_stress": _ffi.RECOVER_STRESS_CAUCHY, "von_mises": _ffi.RECOVER_VON_MISES,
              "energy_density": _ffi.RECOVER_ENERGY_DENSITY, "volume": _ffi.RECOVER_VOLUME}
LOCATIONS = {"points": _ffi.AT_POINTS, "elements": _ffi.AT_ELEMENTS, "nodes": _ffi.AT_NODES}


def _id(table, key, what):
    if isinstance(key, str):
        if key not in table:
            raise ValueError(f"unknown {what} {key!r}: one of {sorted(table)}")
        return table[key]
    return int(key)


def recover(engine: Engine, quantity, where):
    """fh_recover_dev: a float64 torch tensor on the engine's device of shape (rows, *tensor_shape) -- (d, s) for grad_u, (s, d) for
    stress_pk1, (d, d) for strain and cauchy_stress, no trailing axes for the scalars"""
    import torch

    q, w = _id(QUANTITIES, quantity, "quantity"), _id(LOCATIONS, where, "location")
    lib, h = engine._lib, engine._h
    nc, rows = C.c_uint32(0), C.c_uint64(0)
    # one failing call decides the error: the library orders its checks (ids, then the state, then quantity x operator)
    if lib.fh_recover_components(h, q, C.byref(nc)) != _ffi.FH_OK or lib.fh_recover_rows(h, w, C.byref(rows)) != _ffi.FH_OK:
        engine._check(lib.fh_recover_dev(h, q, w, None))
        raise _ffi.FenrisError(_ffi.FH_INVALID_STATE, engine.last_error())
    out = torch.empty(rows.value * nc.value, dtype=torch.float64, device=f"cuda:{engine.device}")
    engine._check(lib.fh_recover_dev(h, q, w, C.c_void_p(out.data_ptr())))
    s = engine.solution_dim()
    if q in (_ffi.RECOVER_GRAD_U, _ffi.RECOVER_STRESS_PK1):
        d = nc.value // s
        shape = (d, s) if q == _ffi.RECOVER_GRAD_U else (s, d)
    elif q in (_ffi.RECOVER_STRAIN, _ffi.RECOVER_STRESS_CAUCHY):
        shape = (s, s)   # (d, d): these exist for the solid operators only, whose s is d
    else:
        shape = ()
    return out.reshape((rows.value,) + shape)


Engine.recover = recover


class Recovery:
    """The named quantities of one engine."""

    def __init__(self, engine: Engine):
        self.engine = engine

    def grad_u(self, where):
        return self.engine.recover("grad_u", where)

    def strain(self, where):
        return self.engine.recover("strain", where)

    def stress_pk1(self, where):
        return self.engine.recover("stress_pk1", where)

    def cauchy_stress(self, where):
        return self.engine.recover("cauchy_stress", where)

    def von_mises(self, where):
        return self.engine.recover("von_mises", where)

    def energy_density(self, where):
        return self.engine.recover("energy_density", where)

    def element_volumes(self):
        return self.engine.recover("volume", "elements")
