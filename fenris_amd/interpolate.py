"""Point location and interpolation at arbitrary points: host mirror of src/space/{spatially_indexed,interpolate,fixed_interpolator}.rs
over fh_locate_points and the fh_interpolator_* calls (include/fenris_hip.h).

    indexed = SpatiallyIndexed.from_space(mesh)
    element, xi = indexed.find_closest_element_and_reference_coords(points)
    values = indexed.interpolate_at_points(points, u, sdim)                       # (m, sdim)
    fixed = FixedInterpolator.from_space_and_points(indexed, points, ValuesOrGradients.Both)
    gradients = fixed.interpolate_gradients(u, sdim)                              # (m, sdim, d): [p, j, i] = d u_j / d x_i

Tri3, Tri6, Tet4, Tet10 and Tet20 meshes.  numpy arrays go through the host entry points; torch tensors on the engine's device stay
there (the _dev entry points) and come back as tensors.  All numerics run in libfenris_hip.so on the GPU; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import enum

import numpy as np

from . import _ffi
from ._ffi import FenrisError
from .mesh import Mesh
from .refinement import Transfer


def _is_torch(x):
    return type(x).__module__.startswith("torch")


class ValuesOrGradients(enum.Enum):
    """ValuesOrGradients (fixed_interpolator.rs:40-64)"""

    Both = 0
    OnlyValues = 1
    OnlyGradients = 2

    def compute_values(self):
        return self is not ValuesOrGradients.OnlyGradients

    def compute_gradients(self):
        return self is not ValuesOrGradients.OnlyValues


def _dev_f64(t, count, what):
    import torch

    if t.dtype != torch.float64 or not t.is_contiguous() or not t.is_cuda or t.numel() != count:
        raise ValueError(f"{what}: a contiguous float64 tensor of {count} values on the engine's device is expected")
    return C.c_void_p(t.data_ptr())


class SpatiallyIndexed:
    """SpatiallyIndexed (spatially_indexed.rs): a mesh on an engine with the point-location index built."""

    def __init__(self, mesh: Mesh, engine, own):
        self.mesh, self.engine, self._own = mesh, engine, own

    @classmethod
    def from_space(cls, mesh: Mesh, engine=None):
        """the mesh becomes the engine's mesh (an Engine(0) of its own without one) and the index is built"""
        own = engine is None
        if own:
            from .assembly import Engine

            engine = Engine(0)
        engine.set_mesh(mesh)
        engine._check(engine._lib.fh_point_index_build(engine._h))
        return cls(mesh, engine, own)

    def space(self):
        return self.mesh

    def close(self):
        if self._own and self.engine is not None:
            self.engine.close()
        self.engine = None

    def locate(self, points):
        """(element, xi, in_element): element is 2^64 - 1 where there is none"""
        eng, d = self.engine, self.mesh.vertices.shape[1]
        if _is_torch(points):
            import torch

            m = points.numel() // d
            elem = torch.empty(m, dtype=torch.int64, device=points.device)
            xi = torch.empty((m, d), dtype=torch.float64, device=points.device)
            ins = torch.empty(m, dtype=torch.uint8, device=points.device)
            eng._check(eng._lib.fh_locate_points_dev(eng._h, _dev_f64(points, m * d, "points"), m, C.c_void_p(elem.data_ptr()),
                                                     C.c_void_p(xi.data_ptr()), C.c_void_p(ins.data_ptr())))
            return elem, xi, ins
        p = _ffi.as_f64(points).reshape(-1, d)
        m = len(p)
        elem = np.zeros(m, dtype=np.uint64)
        xi = np.zeros((m, d))
        ins = np.zeros(m, dtype=np.uint8)
        eng._check(eng._lib.fh_locate_points(eng._h, _ffi.fp(p), m, _ffi.up(elem), _ffi.fp(xi), ins.ctypes.data_as(C.POINTER(C.c_uint8))))
        return elem, xi, ins.astype(bool)

    def find_closest_element_and_reference_coords(self, points):
        """(element indices, reference coordinates) of every point (FindClosestElement, for many points at once)"""
        elem, xi, _ = self.locate(points)
        return elem, xi

    # the on-demand calls are served by a transient interpolator: the same kernels, so the same bits as a fixed one
    def interpolate_at_points(self, points, u, sdim):
        fixed = FixedInterpolator.from_space_and_points(self, points, ValuesOrGradients.OnlyValues)
        try:
            return fixed.interpolate(u, sdim)
        finally:
            fixed.close()

    def interpolate_gradient_at_points(self, points, u, sdim):
        fixed = FixedInterpolator.from_space_and_points(self, points, ValuesOrGradients.OnlyGradients)
        try:
            return fixed.interpolate_gradients(u, sdim)
        finally:
            fixed.close()


def _bad(message):
    return FenrisError(_ffi.FH_BAD_ARGUMENT, message)


class FixedInterpolator:
    """FixedInterpolator (fixed_interpolator.rs): basis values and / or physical gradients of the supporting nodes of fixed points, on the
    device; owns an fh_interpolator."""

    def __init__(self, lib, handle, keep=None):
        self._lib, self._h, self._keep = lib, handle, keep
        m, nnz, d, hv, hg = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_int(), C.c_int()
        self._lib.fh_interpolator_sizes(self._h, C.byref(m), C.byref(nnz), C.byref(d), C.byref(hv), C.byref(hg))
        self.num_points, self.num_indices, self.geometry_dim = int(m.value), int(nnz.value), int(d.value)
        self.has_values, self.has_gradients = bool(hv.value), bool(hg.value)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.fh_interpolator_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != _ffi.FH_OK:
            raise FenrisError(rc, (self._lib.fh_interpolator_last_error(self._h) or b"").decode())

    @classmethod
    def from_space_and_points(cls, indexed: SpatiallyIndexed, points, what=ValuesOrGradients.Both):
        eng, d = indexed.engine, indexed.mesh.vertices.shape[1]
        out = C.c_void_p()
        what = ValuesOrGradients(what)
        if _is_torch(points):
            m = points.numel() // d
            eng._check(eng._lib.fh_interpolator_create_dev(eng._h, _dev_f64(points, m * d, "points"), m, what.value, C.byref(out)))
        else:
            p = _ffi.as_f64(points).reshape(-1, d)
            eng._check(eng._lib.fh_interpolator_create(eng._h, _ffi.fp(p), len(p), what.value, C.byref(out)))
        return cls(eng._lib, out, keep=eng)

    from_space_and_points_par = from_space_and_points   # both run on the device

    @classmethod
    def from_compressed_values(cls, node_values, node_gradients, node_indices, supported_node_offsets, geometry_dim=None, engine=None):
        """from_compressed_values (fixed_interpolator.rs:201-240); its assertions raise FenrisError(FH_BAD_ARGUMENT).  geometry_dim: values
        per gradient (taken from the lengths when not given, as the reference does at the time it interpolates)."""
        idx, off = _ffi.as_u64(node_indices).ravel(), _ffi.as_u64(supported_node_offsets).ravel()
        val = None if node_values is None else _ffi.as_f64(node_values).ravel()
        grad = None if node_gradients is None else _ffi.as_f64(node_gradients).ravel()
        if len(off) == 0:
            raise _bad("supported node offsets must hold at least one entry")
        if np.any(off > len(idx)):
            raise _bad("Supported node offsets must be in bounds with respect to supported nodes.")
        if np.any(off[1:] < off[:-1]):
            raise _bad("supported node offsets must not decrease")
        if val is not None and len(val) != len(idx):
            raise _bad("Number of node values and indices must be the same")
        if grad is not None:
            if len(idx) == 0 and len(grad) != 0:
                raise _bad("gradient data must be empty if indices are empty")
            if len(idx) and len(grad) % len(idx) != 0:
                raise _bad("Number of gradient values must be compatible with number of indices")
        if geometry_dim is None:
            geometry_dim = len(grad) // len(idx) if (grad is not None and len(idx)) else 1
        if geometry_dim not in (1, 2, 3) or (grad is not None and len(grad) != geometry_dim * len(idx)):
            raise _bad("the gradients hold geometry_dim (1, 2 or 3) values per index")
        own = engine is None
        if own:
            from .assembly import Engine

            engine = Engine(0)
        out = C.c_void_p()
        try:
            # (an empty array still has to arrive as a non-null pointer: null means "not given")
            idx_p = idx if len(idx) else np.zeros(1, dtype=np.uint64)
            val_p = val if val is None or len(val) else np.zeros(1)
            grad_p = grad if grad is None or len(grad) else np.zeros(1)
            engine._check(engine._lib.fh_interpolator_from_compressed(
                engine._h, int(geometry_dim), len(off) - 1, _ffi.up(off), _ffi.up(idx_p), len(idx), _ffi.fp(val_p),
                0 if val is None else len(val), _ffi.fp(grad_p), 0 if grad is None else len(grad), C.byref(out)))
        finally:
            if own:
                engine.close()   # the interpolator owns its arrays; it keeps the device and the (null) stream
        return cls(engine._lib, out, keep=None if own else engine)

    def data(self):
        """(supported_node_offsets, node_indices, node_values or None, node_gradients (num_indices, d) or None) copied out"""
        off = np.zeros(self.num_points + 1, dtype=np.uint64)
        idx = np.zeros(self.num_indices, dtype=np.uint64)
        val = np.zeros(self.num_indices) if self.has_values else None
        grad = np.zeros((self.num_indices, self.geometry_dim)) if self.has_gradients else None
        self._check(self._lib.fh_interpolator_data(self._h, _ffi.up(off), _ffi.up(idx) if self.num_indices else None,
                                                   _ffi.fp(val) if self.num_indices else None, _ffi.fp(grad) if self.num_indices else None))
        return off, idx, val, grad

    def _apply(self, u, sdim, gradients):
        m, s, d = self.num_points, int(sdim), self.geometry_dim
        shape = (m, s, d) if gradients else (m, s)
        if _is_torch(u):
            import torch

            out = torch.empty(shape, dtype=torch.float64, device=u.device)
            fn = self._lib.fh_interpolator_apply_gradients_dev if gradients else self._lib.fh_interpolator_apply_dev
            self._check(fn(self._h, s, _dev_f64(u, u.numel(), "u"), u.numel(), C.c_void_p(out.data_ptr())))
            return out
        uh = _ffi.as_f64(u).ravel()
        out = np.zeros(shape)
        fn = self._lib.fh_interpolator_apply_gradients if gradients else self._lib.fh_interpolator_apply
        self._check(fn(self._h, s, _ffi.fp(uh), len(uh), _ffi.fp(out)))
        return out

    def interpolate(self, u, sdim=1):
        """(m, sdim): the field with sdim interleaved components per node, at the points"""
        return self._apply(u, sdim, False)

    def interpolate_gradients(self, u, sdim=1):
        """(m, sdim, d): [p, j, i] = d u_j / d x_i at point p (the reference's d x sdim matrix, column-major)"""
        return self._apply(u, sdim, True)

    def to_transfer(self, num_nodes=None) -> Transfer:
        """the values as a refinement.Transfer by point over the nodes (num_nodes: the largest index + 1 when not given)"""
        off, idx, val, _ = self.data()
        if val is None:
            raise FenrisError(_ffi.FH_INVALID_STATE, "to_transfer: the interpolator holds no values")
        if num_nodes is None:
            num_nodes = int(idx.max()) + 1 if len(idx) else 0
        return Transfer(off, idx, val, int(num_nodes))
