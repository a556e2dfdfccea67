"""Degree coarsening of Tet10, Tri6, Quad9, Hex20 and Hex27 meshes: the linear mesh on their vertex nodes and the transfer from its
vertices to all nodes (fh_coarsen_degree; the convention is in include/fenris_hip.h).  With it a higher-order problem gets a multigrid
hierarchy: the p-coarsening step on top of the linear hierarchies of fenris_amd.refinement (degree_hierarchy).

The opposite direction, elevate_degree (fh_elevate_degree), forms the quadratic mesh over a linear one on the device, numbered and placed
as the host converters of fenris_amd.mesh do, and hands the same transfer out with it: degree_hierarchy_from_linear builds the hierarchy
of a quadratic problem from the linear meshes alone.
"""
from __future__ import annotations

import numpy as np

from . import _ffi
from .mesh import Mesh
from .refinement import _engine_for_call, permute_transfer

DEGREE_KINDS = tuple(_ffi.LINEAR_KIND)


def coarsen_degree_with_transfer(mesh: Mesh, engine=None):
    """(linear mesh, Transfer, vertex_nodes): the linear mesh on the vertex nodes of `mesh` in the order of their indices, cells and
    their nodes in the order of `mesh`; vertex_nodes[j] is the node of `mesh` that became vertex j.  With an engine: its device pass (the
    mesh becomes the engine's mesh).  Without: an Engine(0) of its own for the call."""
    if engine is None and mesh.elem_kind not in DEGREE_KINDS:
        raise _ffi.FenrisError(_ffi.FH_UNSUPPORTED, "degree coarsening is implemented for Tet10, Tri6, Quad9, Hex20 and Hex27 meshes only")
    with _engine_for_call(engine) as eng:
        eng.set_mesh(mesh)
        eng.coarsen_degree()
        return eng.degree_coarsening()


def coarsen_degree(mesh: Mesh, engine=None) -> Mesh:
    """the linear mesh of coarsen_degree_with_transfer"""
    return coarsen_degree_with_transfer(mesh, engine)[0]


def elevate_degree_with_transfer(mesh: Mesh, to_kind, engine=None):
    """(high mesh, Transfer): the Tet10, Tri6, Quad9, Hex20 or Hex27 mesh over the linear `mesh`, bit for bit the mesh of
    tet10_mesh_from_tet4 and its siblings, and the transfer from the vertices of `mesh` to its nodes.  With an engine: its device pass
    (the linear mesh becomes the engine's mesh and the engine holds the elevation: Engine.set_mesh_from_degree_elevation).  Without: an
    Engine(0) of its own for the call."""
    if engine is None and _ffi.LINEAR_KIND.get(to_kind) != mesh.elem_kind:
        code = _ffi.FH_BAD_ARGUMENT if mesh.elem_kind in _ffi.LINEAR_KIND.values() else _ffi.FH_UNSUPPORTED
        raise _ffi.FenrisError(code, "degree elevation goes from Tet4 to Tet10, Tri3 to Tri6, Quad4 to Quad9 and Hex8 to Hex20 or Hex27")
    with _engine_for_call(engine) as eng:
        eng.set_mesh(mesh)
        eng.elevate_degree(to_kind)
        return eng.degree_elevation()


def elevate_degree(mesh: Mesh, to_kind, engine=None) -> Mesh:
    """the high mesh of elevate_degree_with_transfer"""
    return elevate_degree_with_transfer(mesh, to_kind, engine)[0]


def matching_vertex_permutation(new_mesh: Mesh, old_mesh: Mesh, rtol=1e-12):
    """perm[new] = old for two meshes of one kind with the same cells in the same order and the same node order within each cell, read off
    the connectivities.  ValueError when the correspondence is not one-to-one or the positions differ (by more than rtol * max |x|)."""
    if new_mesh.elem_kind != old_mesh.elem_kind:
        raise ValueError("the meshes differ in element kind")
    cn = np.asarray(new_mesh.connectivity).astype(np.int64).ravel()
    co = np.asarray(old_mesh.connectivity).astype(np.int64).ravel()
    n = new_mesh.num_nodes()
    if len(cn) != len(co) or n != old_mesh.num_nodes():
        raise ValueError("the meshes differ in size")
    perm = np.full(n, -1, dtype=np.int64)
    perm[cn] = co
    if (perm < 0).any() or not np.array_equal(perm[cn], co) or len(np.unique(perm)) != n:
        raise ValueError("the vertices of the two meshes do not correspond one to one")
    vn, vo = np.asarray(new_mesh.vertices), np.asarray(old_mesh.vertices)[perm]
    if n and np.abs(vn - vo).max() > rtol * np.abs(vn).max():
        raise ValueError("corresponding vertices of the two meshes differ in position")
    return perm.astype(np.uint64)


def degree_hierarchy(high_mesh: Mesh, linear_meshes, transfers, engine=None):
    """(coarse_meshes, transfers) for GeometricMultigrid(fine_assembler, coarse_meshes, transfers) under a fine assembler on high_mesh.
    linear_meshes (coarsest first) and the transfers between them are what refine_uniformly_repeat_with_transfers returns;
    linear_meshes[-1] has the cells of high_mesh's linear part in any vertex numbering (the converters relabel).  The finest linear level
    becomes the degree coarsening of high_mesh: the fine side of transfers[-1] is permuted to its numbering, and the transfer from it to
    high_mesh is appended.  One linear mesh gives a two-level hierarchy."""
    linear_meshes, transfers = list(linear_meshes), list(transfers)
    if not linear_meshes or len(transfers) != len(linear_meshes) - 1:
        raise ValueError("one transfer between every two consecutive linear meshes")
    linear, p_transfer, _ = coarsen_degree_with_transfer(high_mesh, engine)
    perm = matching_vertex_permutation(linear, linear_meshes[-1])
    if transfers:
        transfers[-1] = permute_transfer(transfers[-1], fine_perm=perm)
    return linear_meshes[:-1] + [linear], transfers + [p_transfer]


def degree_hierarchy_from_linear(linear_meshes, transfers, to_kind, engine=None):
    """(high_mesh, coarse_meshes, transfers): degree_hierarchy from the linear side.  linear_meshes (coarsest first) and the transfers
    between them are what refine_uniformly_repeat_with_transfers returns.  The finest linear mesh is elevated to `to_kind` on the device and
    the elevation's transfer, which is over that mesh's own vertex numbering, is the finest step as it is: no degree coarsening of the
    result, no permutation.  GeometricMultigrid(fine_assembler on high_mesh, coarse_meshes, transfers) takes the rest; with an engine, that
    engine holds the elevation afterwards (Engine.set_mesh_from_degree_elevation hands the high mesh on, device to device)."""
    linear_meshes, transfers = list(linear_meshes), list(transfers)
    if not linear_meshes or len(transfers) != len(linear_meshes) - 1:
        raise ValueError("one transfer between every two consecutive linear meshes")
    high, p_transfer = elevate_degree_with_transfer(linear_meshes[-1], to_kind, engine)
    return high, linear_meshes, transfers + [p_transfer]
