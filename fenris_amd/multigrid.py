"""Geometric multigrid preconditioner of the matrix-free solvers (fh_mg_*, FH_PRECOND_MULTIGRID).

GeometricMultigrid builds one engine per coarse mesh with the fine assembler's operator, uniform quadrature table and data; the
hierarchy itself (fh_mg_create) is made when a solver first uses it with a set of fine Dirichlet nodes, whose coarse sets follow by
injection.  MatrixFreeOperator, MatrixFreeTangent, MatrixFreeShiftedTangent and MatrixFreeNewton take it through with_multigrid.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi
from .assembly import ElementEllipticAssembler, Engine, _is_torch
from .dirichlet import DofSet
from .operators import LinearElasticMaterial, MaterialEllipticOperator


def _injection(transfer):
    """coarse node -> its fine copy (the rows with one parent of weight 1)"""
    off = transfer.offsets.astype(np.int64)
    single = np.where(off[1:] - off[:-1] == 1)[0]
    single = single[transfer.weights[off[single]] == 1.0]
    inj = np.full(transfer.num_coarse, -1, dtype=np.int64)
    inj[transfer.indices[off[single]].astype(np.int64)] = single
    if (inj < 0).any():
        raise _ffi.FenrisError(_ffi.FH_BAD_ARGUMENT, "a coarse node has no injected fine copy")
    return inj


_NONLINEAR = (_ffi.NEO_HOOKEAN, _ffi.STVK, _ffi.STABLE_NEO_HOOKEAN)   # their levels need a u


class GeometricMultigrid:
    """V-cycle preconditioner over coarse_meshes (coarsest first) and transfers (transfers[k]: coarse_meshes[k] -> the next finer mesh, the
    last one -> the fine assembler's mesh; Transfer objects of fenris_amd.refinement).  coarse_operator "tangent": the fine operator on
    every level (NeoHookean, StVK and StableNeoHookean levels receive the fine u by injection at each solve); "linearized": LinearElastic with the same Lame
    data on the coarse levels (the tangent at u = 0).  degree, smoothing_range: the Chebyshev-Jacobi smoother (fh_mg_set_smoother).

    The hierarchy is sized for the meshes its engines hold when it is made: Engine.set_mesh on the fine engine or on a level's engine
    invalidates it, and the multigrid solves and apply then raise FH_INVALID_STATE naming the level (the lifetime rule in fenris_hip.h,
    above fh_mg_create).  Build a new GeometricMultigrid for the new meshes."""

    def __init__(self, fine_assembler, coarse_meshes, transfers, coarse_operator="tangent", degree=3, smoothing_range=15.0, eig_steps=10):
        if coarse_operator not in ("tangent", "linearized"):
            raise ValueError('coarse_operator must be "tangent" or "linearized"')
        if len(coarse_meshes) != len(transfers):
            raise ValueError("one transfer per coarse mesh")
        qt = fine_assembler.qtable
        if hasattr(qt, "rules") or hasattr(qt, "element_to_rule_map") or not hasattr(qt, "weights"):
            raise _ffi.FenrisError(_ffi.FH_UNSUPPORTED, "GeometricMultigrid: the fine assembler needs a UniformQuadratureTable")
        if qt.data is not None and not np.all(np.asarray(qt.data) == np.asarray(qt.data)[:1]):
            raise _ffi.FenrisError(_ffi.FH_UNSUPPORTED, "GeometricMultigrid: the quadrature data must be the same at every point")
        self.fine_assembler = fine_assembler
        self.engine = fine_assembler.engine
        self.degree, self.smoothing_range, self.eig_steps = int(degree), float(smoothing_range), int(eig_steps)
        op = fine_assembler.op
        nonlinear = op.op_kind in _NONLINEAR
        cop = MaterialEllipticOperator(LinearElasticMaterial()) if (coarse_operator == "linearized" and nonlinear) else op
        s = self.engine.solution_dim()
        self.levels = []
        for m in coarse_meshes:
            eng = Engine(self.engine.device)
            u = np.zeros(s * m.num_nodes()) if cop.op_kind in _NONLINEAR else None
            self.levels.append(ElementEllipticAssembler(eng, m, cop, qt, u))
        self.transfers = [self._check_transfer(t, k) for k, t in enumerate(transfers)]
        self._inj = [_injection(t) for t in self.transfers]
        self._h = None
        self._key = None

    def _check_transfer(self, t, k):
        nf = self.levels[k + 1].num_nodes() if k + 1 < len(self.levels) else self.engine.num_nodes()
        if t.num_fine != nf or t.num_coarse != self.levels[k].num_nodes():
            raise ValueError(f"transfer {k} does not match the sizes of its meshes")
        return t

    def _bind(self, fine_nodes, density=None):
        """(re)create the hierarchy for the fine Dirichlet nodes (and, for the shifted map, the density) and attach it to the fine engine"""
        held = fine_nodes if isinstance(fine_nodes, DofSet) else None   # (single components: the masks go down the hierarchy by injection)
        nodes = held.nodes if held is not None else np.zeros(0, dtype=np.uint64) if fine_nodes is None else np.unique(_ffi.as_u64(fine_nodes))
        rho = None if density is None else np.ascontiguousarray(np.atleast_1d(np.asarray(density, dtype=np.float64)).ravel())
        if rho is not None and len(rho) != 1:
            raise _ffi.FenrisError(_ffi.FH_UNSUPPORTED, "GeometricMultigrid: per-element density is not carried to the coarse levels")
        key = (nodes.tobytes() if held is None else held.key(), None if rho is None else rho.tobytes())
        lib = _ffi.lib()
        if self._h is not None and key == self._key:
            self.engine._check(lib.fh_set_multigrid(self.engine._h, self._h))
            return
        self._destroy()
        mask = np.zeros(self.engine.num_nodes(), dtype=bool)
        mask[nodes.astype(np.int64)] = True
        num_fine = self.engine.num_nodes()
        for k in range(len(self.levels) - 1, -1, -1):
            mask = mask[self._inj[k]]
            eng = self.levels[k].engine
            if held is not None:
                held = held.injected(self._inj[k], num_fine)
                num_fine = len(self._inj[k])
                eng.set_operator_dirichlet_nodes(held)
            else:
                eng.set_operator_dirichlet_nodes(np.where(mask)[0].astype(np.uint64))
            if rho is not None:
                eng.set_mass_density(rho)
        self._create()
        self._key = key

    def _create(self):
        lib = _ffi.lib()
        n = len(self.levels)
        ctxs = (C.c_void_p * max(n, 1))(*[lv.engine._h for lv in self.levels])
        keep = [(_ffi.as_u64(t.offsets), _ffi.as_u64(t.indices), _ffi.as_f64(t.weights)) for t in self.transfers]
        offs = (_ffi.u64p * max(n, 1))(*[_ffi.up(a) for a, _, _ in keep])
        idxs = (_ffi.u64p * max(n, 1))(*[_ffi.up(b) for _, b, _ in keep])
        ws = (_ffi.f64p * max(n, 1))(*[_ffi.fp(c) for _, _, c in keep])
        h = C.c_void_p()
        self.engine._check(lib.fh_mg_create(self.engine._h, n, ctxs, offs, idxs, ws, C.byref(h)))
        self._h = h.value
        self.engine._check(lib.fh_mg_set_smoother(self._h, self.degree, self.smoothing_range, self.eig_steps))
        self.engine._check(lib.fh_set_multigrid(self.engine._h, self._h))

    def _destroy(self):
        if self._h is not None:
            lib = _ffi.lib()
            lib.fh_mg_destroy(self._h)
            self._h = None
            self._key = None

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    def apply(self, r, z, alpha=0.0, beta=1.0, dirichlet_nodes=None, density=None):
        """one V-cycle z = B r (device tensors) on alpha M + beta T(u), with the fine engine's current Dirichlet nodes given again here
        (a node list, or a DofSet of fenris_amd.dirichlet for single components)"""
        if not (_is_torch(r) and _is_torch(z)):
            raise TypeError("GeometricMultigrid.apply takes device tensors")
        self.engine.set_operator_dirichlet_nodes(dirichlet_nodes)
        self._bind(dirichlet_nodes, density)
        self.engine._check(_ffi.lib().fh_mg_apply_dev(self._h, float(alpha), float(beta), C.c_void_p(r.data_ptr()), C.c_void_p(z.data_ptr())))
        return z

    def level_info(self, level):
        """(lambda_max of the last setup, dofs) of level `level` (0: the coarsest, len(levels): the fine one)"""
        if self._h is None:
            raise _ffi.FenrisError(_ffi.FH_INVALID_STATE, "the hierarchy has not been set up by a solve yet")
        lam, nd = C.c_double(), C.c_uint64()
        self.engine._check(_ffi.lib().fh_mg_level_info(self._h, int(level), C.byref(lam), C.byref(nd)))
        return float(lam.value), int(nd.value)
