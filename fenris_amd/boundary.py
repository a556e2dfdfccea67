"""Boundary of a mesh and surface loads on it: host mirror of Mesh::find_boundary_faces / find_boundary_vertices /
find_boundary_cells / extract_surface_mesh (src/mesh.rs:154-216, 505-516) over fh_find_boundary_faces and fh_assemble_surface_load.
The search and the load integral run on the device; this module only carries arrays."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _ffi

# the face of a cell kind (FaceConnectivity of src/connectivity.rs) and the corners of that face in its node list
FACE_KIND = {_ffi.QUAD4: "Segment2", _ffi.TRI3: "Segment2", _ffi.QUAD9: "Segment3", _ffi.TRI6: "Segment3", _ffi.TET4: "Tri3",
             _ffi.TET10: "Tri6", _ffi.HEX8: "Quad4", _ffi.HEX20: "Quad8", _ffi.HEX27: "Quad9", _ffi.TET20: None}
FACE_NODES = {"Segment2": 2, "Segment3": 3, "Tri3": 3, "Tri6": 6, "Quad4": 4, "Quad8": 8, "Quad9": 9, None: 0}
_FACE_CORNERS = {"Segment2": [0, 1], "Segment3": [0, 2], "Tri3": [0, 1, 2], "Tri6": [0, 1, 2], "Quad4": [0, 1, 2, 3], "Quad8": [0, 1, 2, 3],
                 "Quad9": [0, 1, 2, 3]}


def _is_torch(x):
    return type(x).__module__.startswith("torch")


@dataclass
class SurfaceMesh:
    """Mesh<f64, D, C::FaceConnectivity>: faces embedded in D dimensions (Tri3 in 3D, Segment2 in 2D, ...).  Not a context mesh: the
    engine's element kinds have no embedded surface elements."""
    vertices: np.ndarray
    connectivity: np.ndarray
    face_kind: Optional[str]

    def num_elements(self):
        return len(self.connectivity)

    def num_nodes(self):
        return len(self.vertices)


class BoundaryFaces:
    """The result of Mesh::find_boundary_faces: per face its nodes in the cell's (outward) orientation, the cell and the local face
    index, in ascending lexicographic order of the sorted node tuples.  Also any subset of it (``select``)."""

    def __init__(self, mesh, face_connectivity, cells, local_faces):
        self.mesh = mesh
        self.face_kind = FACE_KIND[mesh.elem_kind]
        self.face_connectivity = np.ascontiguousarray(face_connectivity, dtype=np.uint64).reshape(-1, max(FACE_NODES[self.face_kind], 1))
        self.cells = np.ascontiguousarray(cells, dtype=np.uint64)
        self.local_faces = np.ascontiguousarray(local_faces, dtype=np.uint32)

    def __len__(self):
        return len(self.cells)

    def __iter__(self):  # (face_connectivity, cells, local_faces), the tuple of the reference
        return iter((self.face_connectivity, self.cells, self.local_faces))

    def _corners(self):
        return self.mesh.vertices[self.face_connectivity[:, _FACE_CORNERS[self.face_kind]].astype(np.int64)]  # F x nc x d

    def centroids(self):
        """mean of the face's corner vertices"""
        return self._corners().mean(axis=1)

    def normals(self):
        """unit outward normals from the face's corners (a quadrilateral: its diagonals' cross product)"""
        x = self._corners()
        if x.shape[2] == 2:
            t = x[:, 1] - x[:, 0]
            a = np.stack([t[:, 1], -t[:, 0]], axis=1)
        elif x.shape[1] == 3:
            a = np.cross(x[:, 1] - x[:, 0], x[:, 2] - x[:, 0])
        else:
            a = np.cross(x[:, 2] - x[:, 0], x[:, 3] - x[:, 1])
        return a / np.linalg.norm(a, axis=1, keepdims=True)

    def select(self, mask_or_predicate):
        """A subset: a boolean mask / index array, or a predicate called with (centroids, normals) returning one."""
        m = mask_or_predicate(self.centroids(), self.normals()) if callable(mask_or_predicate) else mask_or_predicate
        m = np.asarray(m)
        return BoundaryFaces(self.mesh, self.face_connectivity[m], self.cells[m], self.local_faces[m])

    def vertices(self):
        """sorted unique nodes of these faces"""
        return np.unique(self.face_connectivity)


def _engine_for(mesh, engine=None):
    from .assembly import Engine

    eng = engine or Engine()
    eng.set_mesh(mesh)
    return eng


def find_boundary_faces(mesh, engine=None) -> BoundaryFaces:
    eng = _engine_for(mesh, engine)
    fn, cells, lfs = eng.find_boundary_faces()
    return BoundaryFaces(mesh, fn, cells, lfs)


def find_boundary_vertices(mesh, engine=None):
    return _engine_for(mesh, engine).boundary_vertices()


def find_boundary_cells(mesh, engine=None):
    return _engine_for(mesh, engine).boundary_cells()


def extract_surface_mesh(mesh, engine=None) -> SurfaceMesh:
    """mesh.rs:505-516: the boundary faces in search order with their orientation, then keep_cells over all of them (mesh.rs:305-354):
    the vertices in use keep their relative order and are relabelled by rank"""
    eng = _engine_for(mesh, engine)
    fn, _, _ = eng.find_boundary_faces()
    keep = eng.boundary_vertices()
    label = np.zeros(mesh.num_nodes(), dtype=np.uint64)
    label[keep.astype(np.int64)] = np.arange(len(keep), dtype=np.uint64)
    return SurfaceMesh(mesh.vertices[keep.astype(np.int64)].copy(), label[fn.astype(np.int64)], FACE_KIND[mesh.elem_kind])


class SurfaceLoad:
    """The Neumann term of a face list: ``with_traction(t)`` (solution dim 1 or d) or ``with_pressure(p)`` (solution dim d), each a
    constant, a per-face array, a per-(face, point) array or a callable of the physical face points x (F x nq x d).  ``rule`` is
    (weights, points) on the face's reference domain.  An element vector assembler in the sense of VectorAssembler."""

    def __init__(self, space, faces: BoundaryFaces, rule, engine=None):
        self.space, self.faces = space, faces
        self.weights = _ffi.as_f64(rule[0])
        self.points = _ffi.as_f64(rule[1]).reshape(len(self.weights), -1)
        d = _ffi.ELEM_DIM[space.elem_kind]
        if self.points.shape[1] != d - 1:
            raise ValueError("the face rule must have points of dimension d - 1")
        self.engine = _engine_for(space, engine)
        self._kind, self._data, self._sdim = None, None, d

    def _shape(self, v, comps):
        F, nq = len(self.faces), len(self.weights)
        if callable(v):
            v = v(self.engine.physical_face_quadrature_points(self.faces.cells, self.faces.local_faces, self.points))
        v = np.ascontiguousarray(v, dtype=np.float64)
        for count, shape in ((1, (comps,)), (F, (F, comps)), (F * nq, (F, nq, comps))):
            if v.size == count * comps and (v.ndim <= 1 or v.shape == shape or (comps == 1 and v.shape == shape[:-1])):
                return v.reshape(-1), count
        raise ValueError(f"load data must be one value, one per face or one per face and point ({comps} components each)")

    def with_traction(self, t, solution_dim=None):
        d = _ffi.ELEM_DIM[self.space.elem_kind]
        s = solution_dim if solution_dim is not None else (1 if (np.ndim(t) == 0 and not callable(t)) else d)
        if s not in (1, d):
            raise ValueError("solution_dim must be 1 or the geometry dimension")
        self._kind, self._sdim = _ffi.LOAD_TRACTION, s
        self._data = self._shape(t, s)
        return self

    def with_pressure(self, p):
        self._kind, self._sdim = _ffi.LOAD_PRESSURE, _ffi.ELEM_DIM[self.space.elem_kind]
        self._data = self._shape(p, 1)
        return self

    def solution_dim(self):
        return self._sdim

    def num_nodes(self):
        return self.space.num_nodes()

    def num_elements(self):
        return self.space.num_elements()

    def assemble_vector_into_engine(self, output):
        if self._kind is None:
            raise ValueError("no load set: with_traction or with_pressure")
        data, count = self._data
        self.engine.assemble_surface_load(output, self._kind, self._sdim, self.faces.cells, self.faces.local_faces, self.weights, self.points,
                                          data, count)

    def assemble_vector_into(self, output):
        n = self._sdim * self.num_nodes()
        if (output.numel() if _is_torch(output) else len(output)) != n:
            raise ValueError("Output dimensions mismatch")
        self.assemble_vector_into_engine(output)

    def assemble_vector(self):
        out = np.zeros(self._sdim * self.num_nodes())
        self.assemble_vector_into(out)
        return out
