"""Uniform refinement of Tet4, Tri3, Quad4 and Hex8 meshes and the transfer between a coarse mesh and its refinement.

refine_uniformly / refine_uniformly_repeat carry the names of the reference's Tri3 refiners (src/mesh/refinement.rs).  The transfer is
the linear (bi-, trilinear) interpolation from the coarse vertices to the fine ones, as CSR by fine node; it is what GeometricMultigrid
prolongates with, and its transpose is the restriction.  Two paths with one numbering convention (include/fenris_hip.h): the device
refiner of an Engine (fh_refine_uniform, all four kinds) and the host sweep fh_refine_hex8_uniform (Hex8 when no engine is given).
"""
from __future__ import annotations

import contextlib
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _ffi
from .mesh import Mesh


@dataclass
class Transfer:
    """fine i = sum over k in [offsets[i], offsets[i + 1]) of weights[k] * coarse indices[k]"""

    offsets: np.ndarray
    indices: np.ndarray
    weights: np.ndarray
    num_coarse: int

    @property
    def num_fine(self):
        return len(self.offsets) - 1

    def to_scipy(self):
        """the (num_fine x num_coarse) prolongation matrix"""
        import scipy.sparse as sp

        return sp.csr_matrix((self.weights, self.indices.astype(np.int64), self.offsets.astype(np.int64)), shape=(self.num_fine, self.num_coarse))

    def apply(self, coarse):
        """the fine values of a coarse nodal field (num_coarse or num_coarse x s)"""
        coarse = np.asarray(coarse, dtype=np.float64)
        return self.to_scipy() @ coarse


DEVICE_KINDS = (_ffi.TET4, _ffi.TRI3, _ffi.QUAD4, _ffi.HEX8)


@contextlib.contextmanager
def _engine_for_call(engine, needed=True):
    """`engine`, or where there is none and one is needed an Engine(0) of the call's own, closed afterwards"""
    if engine is not None or not needed:
        yield engine
        return
    from .assembly import Engine

    own = Engine(0)
    try:
        yield own
    finally:
        own.close()


def refine_uniformly_with_transfer(mesh: Mesh, engine=None):
    """(fine mesh, Transfer): every cell split uniformly (Tet4, Hex8: 8 children; Tri3, Quad4: 4), coarse vertices first under their own
    indices.  With an engine: its device refiner (the mesh becomes the engine's mesh).  Without: Hex8 takes the host sweep, the other
    kinds an Engine(0) of their own for the call."""
    if engine is not None or mesh.elem_kind != _ffi.HEX8:
        if engine is None and mesh.elem_kind not in DEVICE_KINDS:
            raise _ffi.FenrisError(_ffi.FH_UNSUPPORTED, "uniform refinement is implemented for Tet4, Tri3, Quad4 and Hex8 meshes only")
        with _engine_for_call(engine) as eng:
            eng.set_mesh(mesh)
            eng.refine_uniformly()
            return eng.refinement()
    lib = _ffi.lib()
    v, conn = _ffi.as_f64(mesh.vertices), _ffi.as_u64(mesh.connectivity)
    N, E = mesh.num_nodes(), mesh.num_elements()
    nv, nnz = C.c_uint64(), C.c_uint64()
    cp = conn if E else np.zeros(8, dtype=np.uint64)
    rc = lib.fh_refine_hex8_uniform(_ffi.fp(v), N, _ffi.up(cp), E, None, C.byref(nv), None, None, None, None, C.byref(nnz))
    if rc:
        raise _ffi.FenrisError(rc, "fh_refine_hex8_uniform failed")
    out_v = np.zeros((max(nv.value, 1), 3))
    out_c = np.zeros((max(8 * E, 1), 8), dtype=np.uint64)
    off = np.zeros(nv.value + 1, dtype=np.uint64)
    idx = np.zeros(max(nnz.value, 1), dtype=np.uint64)
    w = np.zeros(max(nnz.value, 1))
    rc = lib.fh_refine_hex8_uniform(_ffi.fp(v), N, _ffi.up(cp), E, _ffi.fp(out_v), C.byref(nv), _ffi.up(out_c), _ffi.up(off), _ffi.up(idx),
                                    _ffi.fp(w), C.byref(nnz))
    if rc:
        raise _ffi.FenrisError(rc, "fh_refine_hex8_uniform failed")
    fine = Mesh(out_v[: nv.value].copy(), out_c[: 8 * E].copy(), _ffi.HEX8)
    return fine, Transfer(off, idx[: nnz.value].copy(), w[: nnz.value].copy(), N)


def refine_uniformly(mesh: Mesh, engine=None) -> Mesh:
    """refine_uniformly (src/mesh/refinement.rs)"""
    return refine_uniformly_with_transfer(mesh, engine)[0]


def _needs_engine(mesh, n):
    """whether n refinements of `mesh` need an engine: one Engine(0) then serves all n levels of a kind that has no host path"""
    return mesh.elem_kind != _ffi.HEX8 and mesh.elem_kind in DEVICE_KINDS and int(n) > 0


def refine_uniformly_repeat(mesh: Mesh, n: int, engine=None) -> Mesh:
    """refine_uniformly_repeat (src/mesh/refinement.rs): n uniform refinements"""
    with _engine_for_call(engine, _needs_engine(mesh, n)) as eng:
        for _ in range(int(n)):
            mesh = refine_uniformly(mesh, eng)
    return mesh


def refine_uniformly_repeat_with_transfers(mesh: Mesh, n: int, engine=None):
    """(meshes, transfers): meshes[0] is the input, meshes[k + 1] refines meshes[k] through transfers[k] (coarsest first)"""
    meshes, transfers = [mesh], []
    with _engine_for_call(engine, _needs_engine(mesh, n)) as eng:
        for _ in range(int(n)):
            fine, t = refine_uniformly_with_transfer(meshes[-1], eng)
            meshes.append(fine)
            transfers.append(t)
    return meshes, transfers


def permute_transfer(transfer: Transfer, fine_perm=None, coarse_perm=None) -> Transfer:
    """the transfer after the fine and / or the coarse mesh were renumbered with a vertex Permutation (perm[new] = old, as
    reorder_mesh_par's vertex_permutation()): rows follow the fine order, indices name the new coarse vertices, each row's parents stay
    in ascending (new) index"""
    off = transfer.offsets.astype(np.int64)
    idx = transfer.indices.astype(np.int64)
    w = transfer.weights
    nf = len(off) - 1
    rows = np.arange(nf) if fine_perm is None else np.asarray(fine_perm.perm() if hasattr(fine_perm, "perm") else fine_perm, dtype=np.int64)
    if len(rows) != nf:
        raise ValueError("fine permutation and transfer differ in size")
    if coarse_perm is not None:
        cp = np.asarray(coarse_perm.perm() if hasattr(coarse_perm, "perm") else coarse_perm, dtype=np.int64)
        inv = np.empty(len(cp), dtype=np.int64)
        inv[cp] = np.arange(len(cp))
        idx = inv[idx]
    counts = off[1:] - off[:-1]
    new_counts = counts[rows]
    new_off = np.zeros(nf + 1, dtype=np.int64)
    np.cumsum(new_counts, out=new_off[1:])
    src = np.repeat(off[rows], new_counts) + (np.arange(new_off[-1]) - np.repeat(new_off[:-1], new_counts))
    new_idx, new_w = idx[src], w[src]
    # parents in ascending index within each row
    order = np.lexsort((new_idx, np.repeat(np.arange(nf), new_counts)))
    return Transfer(new_off.astype(np.uint64), new_idx[order].astype(np.uint64), np.ascontiguousarray(new_w[order]), transfer.num_coarse)
