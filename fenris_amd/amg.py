"""Smoothed-aggregation algebraic multigrid for PCG on the assembled matrix (fh_amg_*, FH_PRECOND_AMG).

SmoothedAggregationAMG builds the hierarchy on the device from an element assembler's engine (its pattern) and an assembled CsrMatrix of
that pattern.  Engine.cg_solve(values, b, x, PRECOND_AMG) and ConjugateGradient.with_preconditioner(amg) use it; the values passed to a
solve must be the ones the hierarchy was built from or last refreshed with (update).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi
from .assembly import _is_torch


def _device_values(engine, csr):
    import torch

    v = csr.values if hasattr(csr, "values") else csr
    if _is_torch(v):
        return v
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(f"cuda:{engine.device}")


class SmoothedAggregationAMG:
    """near_nullspace: "rigid_body" (translations and rotations; solution dim = geometry dim), "constant" (one unit translation per
    component) or an array of shape (s N, nb), nb <= 6.  theta: strength threshold; max_levels: levels including the fine one; degree,
    smoothing_range, eig_steps: the Chebyshev-Jacobi smoother (fh_amg_set_smoother).

    The constructor attaches the hierarchy to the engine (fh_set_amg).  An engine holds one hierarchy: attaching another one (a second
    SmoothedAggregationAMG on the same Engine) or closing the engine orphans this one, and every later call on it (apply, update,
    level_info, use as a preconditioner) raises FH_BAD_ARGUMENT.  Build a new one instead.

    The hierarchy holds the engine's pattern: a new mesh on the engine (Engine.set_mesh, a new assembler on it) followed by a pattern
    build, or an operator of another solution dim, invalidates it, and apply, update and the AMG solves then raise FH_INVALID_STATE (the
    lifetime rule in fenris_hip.h, above fh_mg_create).  Build a new one for the new mesh."""

    def __init__(self, element_assembler, csr, near_nullspace="rigid_body", theta=0.0, max_levels=10, degree=3, smoothing_range=15.0,
                 eig_steps=10):
        self.engine = element_assembler.engine
        self._values = _device_values(self.engine, csr)
        B, nb = None, 0
        if isinstance(near_nullspace, str):
            kinds = {"constant": _ffi.AMG_CONSTANT, "rigid_body": _ffi.AMG_RIGID_BODY}
            if near_nullspace not in kinds:
                raise ValueError('near_nullspace must be "rigid_body", "constant" or an array')
            kind = kinds[near_nullspace]
        else:
            kind = _ffi.AMG_USER
            B = np.ascontiguousarray(np.asarray(near_nullspace, dtype=np.float64))
            if B.ndim != 2:
                raise ValueError("near_nullspace array must be (s N, nb)")
            nb = B.shape[1]
            if B.shape[0] != self.engine.solution_dim() * self.engine.num_nodes():
                raise ValueError("near_nullspace array must have s N rows")
        self._B = B
        h = C.c_void_p()
        lib = _ffi.lib()
        self.engine._check(lib.fh_amg_create(self.engine._h, C.c_void_p(self._values.data_ptr()), kind, _ffi.fp(B), nb, float(theta),
                                             int(max_levels), C.byref(h)))
        self._h = h.value
        if (degree, smoothing_range, eig_steps) != (3, 15.0, 10):
            self.engine._check(lib.fh_amg_set_smoother(self._h, int(degree), float(smoothing_range), int(eig_steps)))
        self.engine._check(lib.fh_set_amg(self.engine._h, self._h))
        self.num_levels = 0
        while lib.fh_amg_level_info(self._h, self.num_levels, None, None, None, None) == 0:
            self.num_levels += 1

    def _attach(self):
        self.engine._check(_ffi.lib().fh_set_amg(self.engine._h, self._h))

    def update(self, csr):
        """numeric refresh for new values on the same pattern (aggregates, T and patterns kept)"""
        values = _device_values(self.engine, csr)
        self.engine._check(_ffi.lib().fh_amg_update_values(self._h, C.c_void_p(values.data_ptr())))
        self._values = values
        return self

    def apply(self, r, z):
        """one V-cycle z = B r (device tensors)"""
        if not (_is_torch(r) and _is_torch(z)):
            raise TypeError("SmoothedAggregationAMG.apply takes device tensors")
        self.engine._check(_ffi.lib().fh_amg_apply_dev(self._h, C.c_void_p(r.data_ptr()), C.c_void_p(z.data_ptr())))
        return z

    def level_info(self, level):
        """dict(num_dofs, nnz_blocks, block_size, lambda_max) of level `level` (0: the fine one)"""
        nd, nz, bs, lam = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_double()
        self.engine._check(_ffi.lib().fh_amg_level_info(self._h, int(level), C.byref(nd), C.byref(nz), C.byref(bs), C.byref(lam)))
        return {"num_dofs": int(nd.value), "nnz_blocks": int(nz.value), "block_size": int(bs.value), "lambda_max": float(lam.value)}

    def aggregates(self, level=0):
        """aggregate of every node of `level` (-1: isolated)"""
        n = self.level_info(level)["num_dofs"] // self.level_info(level)["block_size"]
        out = np.zeros(n, dtype=np.uint64)
        self.engine._check(_ffi.lib().fh_amg_aggregates(self._h, int(level), _ffi.up(out)))
        a = out.astype(np.int64)
        a[out == np.iinfo(np.uint64).max] = -1
        return a

    def level_matrix(self, level, which="A"):
        """A, P, T (the tentative prolongator) or B (the level's near-nullspace) of `level` as a scipy CSR matrix"""
        import scipy.sparse as sp

        w = {"A": 0, "P": 1, "T": 2, "B": 3}[which]
        lib = _ffi.lib()
        nnz = C.c_uint64()
        self.engine._check(lib.fh_amg_level_matrix(self._h, int(level), w, None, None, None, C.byref(nnz)))
        info = self.level_info(level)
        rows = info["num_dofs"]
        ci = np.zeros(max(nnz.value, 1), dtype=np.uint64)
        v = np.zeros(max(nnz.value, 1))
        ro = np.zeros(rows + 1, dtype=np.uint64)
        self.engine._check(lib.fh_amg_level_matrix(self._h, int(level), w, _ffi.up(ro), _ffi.up(ci), _ffi.fp(v), C.byref(nnz)))
        if w == 3:
            ncols = self.level_info(1)["block_size"] if self.num_levels > 1 else int(ci[: nnz.value].max()) + 1 if nnz.value else 0
        else:
            ncols = rows if w == 0 else self.level_info(level + 1)["num_dofs"]
        n = int(nnz.value)
        return sp.csr_matrix((v[:n], ci[:n].astype(np.int64), ro.astype(np.int64)), shape=(rows, ncols))

    def operator_complexity(self):
        """sum of the levels' scalar nonzeros over the fine level's"""
        nz = [self.level_info(l)["nnz_blocks"] * self.level_info(l)["block_size"] ** 2 for l in range(self.num_levels)]
        return sum(nz) / nz[0]

    def close(self):
        if getattr(self, "_h", None) is not None:
            _ffi.lib().fh_amg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
