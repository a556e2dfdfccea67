"""Global / local assembly: host mirror of src/assembly/{local,global}.rs over the C ABI.

Names and call shapes follow the reference so that tests read like the reference's own tests:

    quadrature = UniformQuadratureTable.from_points_and_weights(points, weights)
    assembler = (ElementEllipticAssemblerBuilder()
                 .with_finite_element_space(mesh).with_operator(LaplaceOperator())
                 .with_quadrature_table(quadrature).with_u(u).build())
    a_global = CsrAssembler().assemble(assembler)                  # examples/poisson2d.rs:33-60
    colors = color_nodes(mesh); CsrParAssembler().assemble(colors, assembler)

All numerics run in libfenris_hip.so on the GPU; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import types
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _ffi
from . import contact as _contact
from . import dirichlet as _dirichlet
from .compose import _Composable, is_composed
from . import compose as _compose
from ._ffi import (ASSEMBLE_OVERWRITE, SCATTER_ATOMIC, SCATTER_COLORED, SCATTER_GATHER, FenrisError,
                   SingularJacobianError)
from .mesh import Mesh


# ------------------------------------------------------------------------------------------ engine
@dataclass(frozen=True)
class _Held:
    """what an Engine remembers of a derived mesh and its transfer that the library holds on the device"""

    kind: int
    num_nodes: int
    num_cells: int
    nnz: int
    num_rows: int  # of the transfer
    num_coarse: int  # its columns


class Engine:
    """Owns one fh_ctx (one device, one stream)."""

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        self._lib = _ffi.lib()
        self._h = self._lib.fh_create(device)
        if not self._h:
            raise FenrisError(_ffi.FH_HIP_ERROR, f"cannot create a context on HIP device {device} (no GPU?)")
        self.device = device
        if stream is not None:
            self._check(self._lib.fh_set_stream(self._h, C.c_void_p(stream)))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.fh_destroy(self._h)
            self._h = None
            self._sdf_grids = {}   # (the uploads of fenris_amd.contact.SdfGrid went with the context)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_error(self):
        """fh_last_error: the message of the last failed call on this context"""
        return (self._lib.fh_last_error(self._h) or b"").decode()

    def _check(self, rc, failed=None):
        if rc == _ffi.FH_OK:
            return
        msg = (self._lib.fh_last_error(self._h) or b"").decode()
        if rc == _ffi.FH_SINGULAR_JACOBIAN:
            raise SingularJacobianError(msg, int(failed.value) if failed is not None else -1)
        raise FenrisError(rc, msg)

    # inputs
    def set_mesh(self, mesh: Mesh):
        self._mesh = mesh  # keep the host arrays alive
        self._mf_bound = None  # fh_set_mesh clears the operator's Dirichlet nodes
        self._mass_bound = None  # ... and the mass density
        self._contact_bound = None  # ... and the obstacles of the penalty contact term
        self._drop_held()  # ... and drops a held refinement, degree coarsening and degree elevation
        self._check(self._lib.fh_set_mesh(self._h, mesh.elem_kind, _ffi.fp(mesh.vertices), mesh.num_nodes(),
                                          _ffi.up(mesh.connectivity), mesh.num_elements()))

    def set_connectivity_ragged(self, sdim, num_nodes, elem_offsets, elem_nodes):
        eo, en = _ffi.as_u64(elem_offsets), _ffi.as_u64(elem_nodes)
        en_p = en if len(en) else np.zeros(1, dtype=np.uint64)
        self._mf_bound = None
        self._mass_bound = None
        self._contact_bound = None
        self._drop_held()
        self._check(self._lib.fh_set_connectivity_ragged(self._h, sdim, num_nodes, _ffi.up(eo), _ffi.up(en_p), len(eo) - 1))

    def set_active_elements(self, mask):
        """Numerics only over elements with mask != 0; the pattern still comes from all elements."""
        if mask is None:
            self._check(self._lib.fh_set_active_elements(self._h, None))
        else:
            m = np.ascontiguousarray(mask, dtype=np.uint8)
            assert len(m) == self.num_elements()
            self._check(self._lib.fh_set_active_elements(self._h, m.ctypes.data_as(C.c_char_p)))

    def set_row_range(self, node_begin, node_end):
        """owner-computes assembly of the rows of nodes [node_begin, node_end) only (fh_set_row_range)"""
        self._check(self._lib.fh_set_row_range(self._h, int(node_begin), int(node_end)))

    def set_operator(self, op_kind):
        self._check(self._lib.fh_set_operator(self._h, op_kind))

    def set_operator_tensor(self, tensors, symmetric):
        """fh_set_operator_tensor: (nq, d^4) coefficient tensors of FH_TENSOR for the quadrature table in use"""
        t = _ffi.as_f64(tensors)
        self._check(self._lib.fh_set_operator_tensor(self._h, _ffi.fp(t), t.shape[0], 1 if symmetric else 0))

    def set_quadrature_uniform(self, weights, points, params=None):
        w, p = _ffi.as_f64(weights), _ffi.as_f64(points)
        q = None if params is None else _ffi.as_f64(params)
        self._check(self._lib.fh_set_quadrature_uniform(self._h, _ffi.fp(w), _ffi.fp(p), len(w), _ffi.fp(q)))

    def set_quadrature_table(self, qtable):
        """UniformQuadratureTable or CompactQuadratureTable"""
        if hasattr(qtable, "rules"):  # rule-set table: grouped and walked inside the library (fh_set_quadrature_rules)
            rules = qtable.rules
            offs = np.zeros(len(rules) + 1, dtype=np.uint64)
            offs[1:] = np.cumsum([len(r[0]) for r in rules])
            w = np.ascontiguousarray(np.concatenate([r[0] for r in rules]), dtype=np.float64)
            p = np.ascontiguousarray(np.concatenate([np.asarray(r[1], dtype=np.float64).reshape(len(r[0]), -1) for r in rules]))
            has_d = [r[2] is not None for r in rules]
            if any(has_d) and not all(has_d):
                raise ValueError("either every rule carries data or none does")
            d = np.ascontiguousarray(np.concatenate([r[2] for r in rules]), dtype=np.float64) if all(has_d) else None
            emap = _ffi.as_u64(qtable.element_to_rule_map)
            self._keep_q = (offs, w, p, d, emap)
            self._check(self._lib.fh_set_quadrature_rules(self._h, len(rules), _ffi.up(offs), _ffi.fp(w), _ffi.fp(p), _ffi.fp(d),
                                                          _ffi.up(emap)))
        elif hasattr(qtable, "rule_params"):
            w, p = _ffi.as_f64(qtable.weights), _ffi.as_f64(qtable.points)
            self._keep_q = (w, p, qtable.rule_params, qtable.element_to_rule_map)
            self._check(self._lib.fh_set_quadrature_compact(self._h, _ffi.fp(w), _ffi.fp(p), len(w), len(qtable.rule_params),
                                                            _ffi.fp(qtable.rule_params), _ffi.up(qtable.element_to_rule_map)))
        else:
            self.set_quadrature_uniform(qtable.weights, qtable.points, qtable.data)

    def update_vertices(self, vertices):
        """new coordinates for the mesh that is set (same connectivity: pattern and topology tables stay)"""
        self._check(self._lib.fh_update_vertices(self._h, _ffi.fp(_ffi.as_f64(np.ascontiguousarray(vertices)))))

    def set_u(self, u):
        if u is None:
            self._check(self._lib.fh_set_u(self._h, None))
        elif _is_torch(u):
            self._check(self._lib.fh_set_u_dev(self._h, C.c_void_p(u.data_ptr())))
        else:
            self._check(self._lib.fh_set_u(self._h, _ffi.fp(_ffi.as_f64(u))))

    # queries
    def solution_dim(self):
        return int(self._lib.fh_solution_dim(self._h))

    def num_elements(self):
        return int(self._lib.fh_num_elements(self._h))

    def num_nodes(self):
        return int(self._lib.fh_num_nodes(self._h))

    def num_rows(self):
        return int(self._lib.fh_num_rows(self._h))

    def nnz(self):
        return int(self._lib.fh_nnz(self._h))

    def last_kernel_name(self):
        return (self._lib.fh_last_kernel_name(self._h) or b"").decode()

    def synchronize(self):
        self._check(self._lib.fh_synchronize(self._h))

    def set_affine_tolerance(self, rel_tol: float):
        """fh_set_affine_tolerance: 0 switches the affine-element fast path off."""
        self._check(self._lib.fh_set_affine_tolerance(self._h, float(rel_tol)))

    def affine_stats(self):
        """(elements found affine, node blocks on the affine kernel, node blocks on the general kernels)"""
        a, b, g = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.fh_affine_stats(self._h, C.byref(a), C.byref(b), C.byref(g)))
        return int(a.value), int(b.value), int(g.value)

    def vector_tiles_stats(self):
        """fh_vector_tiles_stats: (tiles, partials, largest number of distinct nodes of a tile, longest partial list of a node)"""
        t, p, mt, mp = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.fh_vector_tiles_stats(self._h, C.byref(t), C.byref(p), C.byref(mt), C.byref(mp)))
        return int(t.value), int(p.value), int(mt.value), int(mp.value)

    def affine_shared_stats(self):
        """fh_affine_shared_stats: {"shared", "records", "lists", "reason"} of the last affine sweep"""
        on, nrec, nvec, why = C.c_int(0), C.c_uint64(0), C.c_uint64(0), C.c_char_p()
        self._check(self._lib.fh_affine_shared_stats(self._h, C.byref(on), C.byref(nrec), C.byref(nvec), C.byref(why)))
        return {"shared": bool(on.value), "records": int(nrec.value), "lists": int(nvec.value), "reason": (why.value or b"").decode()}

    def affine_slot_elements(self):
        """fh_affine_slot_elements (internal, for tests): int32 array [node blocks of the affine kernel, slots] of element ids, -1 for an empty slot"""
        us, npos = C.c_int(0), C.c_uint64(0)
        self._check(self._lib.fh_affine_slot_elements(self._h, C.byref(us), C.byref(npos), None))
        out = np.empty((int(npos.value), int(us.value)), dtype=np.int32)
        if out.size:
            self._check(self._lib.fh_affine_slot_elements(self._h, C.byref(us), C.byref(npos), C.c_void_p(out.ctypes.data)))
        return out

    # pattern
    def pattern(self, want_cols=True):
        R = self.num_rows()
        ro = np.zeros(R + 1, dtype=np.uint64)
        nnz = C.c_uint64()
        self._check(self._lib.fh_pattern(self._h, _ffi.up(ro), C.byref(nnz)))
        if not want_cols:
            return ro, None
        ci = np.zeros(max(int(nnz.value), 1), dtype=np.uint64)
        self._check(self._lib.fh_pattern_cols(self._h, _ffi.up(ci)))
        return ro, ci[: int(nnz.value)]

    def build_pattern(self):
        nnz = C.c_uint64()
        self._check(self._lib.fh_pattern(self._h, None, C.byref(nnz)))
        return int(nnz.value)

    def pattern_dev(self, row_offsets_t=None, col_indices_t=None):
        self._check(self._lib.fh_pattern_dev(self._h, _ptr(row_offsets_t), _ptr(col_indices_t)))

    # colouring
    def color(self):
        E = self.num_elements()
        nc = C.c_uint64()
        co = np.zeros(E + 2, dtype=np.uint64)
        lab = np.zeros(max(E, 1), dtype=np.uint64)
        self._check(self._lib.fh_color(self._h, C.byref(nc), _ffi.up(co), _ffi.up(lab)))
        return DisjointSubsetsColors(co[: nc.value + 1].copy(), lab[:E].copy())

    def color_parallel(self):
        """fh_color_parallel: a valid element colouring computed on the device (not the reference's sequential greedy one)"""
        E = self.num_elements()
        nc = C.c_uint64()
        co = np.zeros(E + 2, dtype=np.uint64)
        lab = np.zeros(max(E, 1), dtype=np.uint64)
        self._check(self._lib.fh_color_parallel(self._h, C.byref(nc), _ffi.up(co), _ffi.up(lab)))
        return DisjointSubsetsColors(co[: nc.value + 1].copy(), lab[:E].copy())

    def set_colors(self, colors: "DisjointSubsetsColors"):
        co, lab = _ffi.as_u64(colors.color_offsets), _ffi.as_u64(colors.labels)
        lab_p = lab if len(lab) else np.zeros(1, dtype=np.uint64)
        self._check(self._lib.fh_set_colors(self._h, len(co) - 1, _ffi.up(co), _ffi.up(lab_p)))

    # numeric
    def assemble_matrix(self, values, flags=SCATTER_ATOMIC):
        failed = C.c_uint64(0)
        if _is_torch(values):
            rc = self._lib.fh_assemble_matrix_dev(self._h, C.c_void_p(values.data_ptr()), flags, C.byref(failed))
        else:
            assert values.dtype == np.float64 and values.flags.c_contiguous
            rc = self._lib.fh_assemble_matrix(self._h, _ffi.fp(values), flags, C.byref(failed))
        self._check(rc, failed)

    def assemble_matrix_async(self, values_t, flags):
        self._check(self._lib.fh_assemble_matrix_async_dev(self._h, C.c_void_p(values_t.data_ptr()), flags))

    def set_option(self, name, value):
        """fh_set_option: a FENRIS_HIP_* switch of this context (value None removes it)"""
        self._check(self._lib.fh_set_option(self._h, name.encode(), None if value is None else str(value).encode()))

    def time_assembly(self, values_t, flags, reps=3):
        """fh_time_assembly_dev: milliseconds per assembly (events on the context's stream), after one untimed assembly"""
        ms = C.c_double(0.0)
        self._check(self._lib.fh_time_assembly_dev(self._h, C.c_void_p(values_t.data_ptr()), flags, int(reps), C.byref(ms)))
        return float(ms.value)

    def tune_placement(self, values_t, flags, tries=3):
        """fh_tune_placement_dev: the better of several allocations of the library's own streamed buffer; (ms before, ms after)"""
        a, b = C.c_double(0.0), C.c_double(0.0)
        self._check(self._lib.fh_tune_placement_dev(self._h, C.c_void_p(values_t.data_ptr()), flags, int(tries), C.byref(a), C.byref(b)))
        return float(a.value), float(b.value)

    def assemble_matrix_rows_async(self, values_t, flags, node_begin, node_end):
        """rows of the nodes [node_begin, node_end) only, with the context's second set of tables (fh_assemble_matrix_rows_async_dev)"""
        self._check(self._lib.fh_assemble_matrix_rows_async_dev(self._h, C.c_void_p(values_t.data_ptr()), flags,
                                                                C.c_uint64(int(node_begin)), C.c_uint64(int(node_end))))

    def assemble_matrix_rows(self, values_t, flags, node_begin, node_end):
        failed = C.c_uint64(0)
        self._check(self._lib.fh_assemble_matrix_rows_dev(self._h, C.c_void_p(values_t.data_ptr()), flags,
                                                          C.c_uint64(int(node_begin)), C.c_uint64(int(node_end)), C.byref(failed)), failed)

    def poll_status(self):
        failed = C.c_uint64(0)
        self._check(self._lib.fh_poll_status(self._h, C.byref(failed)), failed)

    def assemble_vector(self, out):
        failed = C.c_uint64(0)
        if _is_torch(out):
            rc = self._lib.fh_assemble_vector_dev(self._h, C.c_void_p(out.data_ptr()), C.byref(failed))
        else:
            rc = self._lib.fh_assemble_vector(self._h, _ffi.fp(out), C.byref(failed))
        self._check(rc, failed)

    def assemble_vector_async(self, out):
        """fh_assemble_vector_async_dev: enqueue only (device tensor); poll_status() reports a singular element"""
        self._check(self._lib.fh_assemble_vector_async_dev(self._h, C.c_void_p(out.data_ptr())))

    def assemble_source_vector(self, out, solution_dim, g=None, values=None):
        """fh_assemble_source_vector(_dev): out += sum_q w |det J| f phi (source.rs:219-278)"""
        gp = _ffi.fp(np.ascontiguousarray(g, dtype=np.float64)) if g is not None else None
        if _is_torch(out):
            vp = C.c_void_p(values.data_ptr()) if values is not None else None
            rc = self._lib.fh_assemble_source_vector_dev(self._h, solution_dim, gp, vp, C.c_void_p(out.data_ptr()))
        else:
            vp = _ffi.fp(np.ascontiguousarray(values, dtype=np.float64)) if values is not None else None
            rc = self._lib.fh_assemble_source_vector(self._h, solution_dim, gp, vp, _ffi.fp(out))
        self._check(rc)

    def physical_quadrature_points(self, nq):
        d = _ffi.ELEM_DIM[self._mesh.elem_kind]
        x = np.zeros((self.num_elements(), nq, d))
        self._check(self._lib.fh_physical_quadrature_points(self._h, _ffi.fp(x)))
        return x

    # boundary of the mesh (fh_find_boundary_faces and its queries) and surface loads on face lists
    def find_boundary_faces(self):
        """Mesh::find_boundary_faces (mesh.rs:167-203) -> (face_nodes F x nf, cells F, local_faces F)"""
        nf, npf = C.c_uint64(0), C.c_uint32(0)
        self._check(self._lib.fh_find_boundary_faces(self._h, C.byref(nf), C.byref(npf)))
        F, k = int(nf.value), int(npf.value)
        fn = np.zeros((F, max(k, 1)), dtype=np.uint64)
        cells, lfs = np.zeros(F, dtype=np.uint64), np.zeros(F, dtype=np.uint32)
        if F:
            self._check(self._lib.fh_boundary_faces(self._h, _ffi.up(fn), _ffi.up(cells), lfs.ctypes.data_as(_ffi.u32p)))
        return fn, cells, lfs

    # meshes derived on the device and held on the engine, side by side, until the next call of the same kind or set_mesh
    def _drop_held(self):
        """the library drops what the engine holds with the mesh"""
        self._refined = self._coarsened = self._elevated = None

    def _fetch_held(self, held, mesh_fn, transfer_fn, with_vertex_nodes=False):
        """a held mesh and its transfer as host arrays -> (Mesh, Transfer[, vertex_nodes])"""
        from .refinement import Transfer

        if held is None:
            self._check(mesh_fn(self._h, *([None] * (3 if with_vertex_nodes else 2))))   # FH_INVALID_STATE
        v = np.zeros((held.num_nodes, _ffi.ELEM_DIM[held.kind]))
        conn = np.zeros((held.num_cells, _ffi.ELEM_NODES[held.kind]), dtype=np.uint64)
        extra = (np.zeros(held.num_nodes, dtype=np.uint64),) if with_vertex_nodes else ()
        off, idx, w = np.zeros(held.num_rows + 1, dtype=np.uint64), np.zeros(held.nnz, dtype=np.uint64), np.zeros(held.nnz)
        self._check(mesh_fn(self._h, _ffi.fp(v), _ffi.up(conn), *[_ffi.up(x) for x in extra]))
        self._check(transfer_fn(self._h, _ffi.up(off), _ffi.up(idx), _ffi.fp(w)))
        return (Mesh(v, conn, held.kind), Transfer(off, idx, w, held.num_coarse)) + extra

    def _adopt_held(self, fn, other: "Engine", held):
        """this engine's mesh becomes the mesh `other` holds, device to device"""
        self._mf_bound = None
        self._mass_bound = None
        self._contact_bound = None
        self._check(fn(self._h, other._h))
        # no host arrays were given: what the engine's own methods ask of a mesh
        self._mesh = types.SimpleNamespace(elem_kind=held.kind, num_nodes=lambda: held.num_nodes, num_elements=lambda: held.num_cells)
        self._drop_held()

    # uniform refinement on the device (fh_refine_uniform): Tet4, Tri3, Quad4, Hex8
    def refine_uniformly(self):
        """refine the engine's mesh; the result stays on the engine until the next refinement or set_mesh.
        -> (num_vertices, num_cells, transfer nnz)"""
        nv, nc, nnz = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self._lib.fh_refine_uniform(self._h, C.byref(nv), C.byref(nc), C.byref(nnz)))
        self._refined = _Held(self._mesh.elem_kind, int(nv.value), int(nc.value), int(nnz.value), int(nv.value), self._mesh.num_nodes())
        return int(nv.value), int(nc.value), int(nnz.value)

    def refinement(self):
        """the held refinement as host arrays -> (Mesh, Transfer)"""
        return self._fetch_held(getattr(self, "_refined", None), self._lib.fh_refinement_mesh, self._lib.fh_refinement_transfer)

    def set_mesh_from_refinement(self, coarse_engine: "Engine"):
        """fh_set_mesh_from_refinement: this engine's mesh becomes the refinement `coarse_engine` holds, device to device"""
        self._adopt_held(self._lib.fh_set_mesh_from_refinement, coarse_engine, getattr(coarse_engine, "_refined", None))

    # degree coarsening on the device (fh_coarsen_degree): Tet10, Tri6, Quad9, Hex20, Hex27 -> the linear mesh on their vertex nodes
    def coarsen_degree(self):
        """coarsen the engine's mesh to its linear kind; the result stays on the engine until the next coarsening or set_mesh.
        -> (num_vertices, transfer nnz)"""
        nv, nnz = C.c_uint64(0), C.c_uint64(0)
        self._coarsened = None
        self._check(self._lib.fh_coarsen_degree(self._h, C.byref(nv), C.byref(nnz)))
        self._coarsened = _Held(_ffi.LINEAR_KIND[self._mesh.elem_kind], int(nv.value), self._mesh.num_elements(), int(nnz.value),
                                self._mesh.num_nodes(), int(nv.value))
        return int(nv.value), int(nnz.value)

    def degree_coarsening(self):
        """the held degree coarsening as host arrays -> (linear Mesh, Transfer, vertex_nodes)"""
        return self._fetch_held(getattr(self, "_coarsened", None), self._lib.fh_degree_coarsening_mesh, self._lib.fh_degree_coarsening_transfer,
                                with_vertex_nodes=True)

    def set_mesh_from_degree_coarsening(self, high_engine: "Engine"):
        """fh_set_mesh_from_degree_coarsening: this engine's mesh becomes the degree coarsening `high_engine` holds, device to device"""
        self._adopt_held(self._lib.fh_set_mesh_from_degree_coarsening, high_engine, getattr(high_engine, "_coarsened", None))

    # degree elevation on the device (fh_elevate_degree): Tet4 -> Tet10, Tri3 -> Tri6, Quad4 -> Quad9, Hex8 -> Hex20 or Hex27
    def elevate_degree(self, to_kind):
        """elevate the engine's linear mesh to `to_kind`; the result stays on the engine until the next elevation or set_mesh.
        -> (num_vertices, transfer nnz)"""
        nv, nnz = C.c_uint64(0), C.c_uint64(0)
        self._elevated = None
        self._check(self._lib.fh_elevate_degree(self._h, int(to_kind), C.byref(nv), C.byref(nnz)))
        self._elevated = _Held(int(to_kind), int(nv.value), self._mesh.num_elements(), int(nnz.value), int(nv.value), self._mesh.num_nodes())
        return int(nv.value), int(nnz.value)

    def degree_elevation(self):
        """the held degree elevation as host arrays -> (high Mesh, Transfer from the linear vertices to its nodes)"""
        return self._fetch_held(getattr(self, "_elevated", None), self._lib.fh_degree_elevation_mesh, self._lib.fh_degree_elevation_transfer)

    def set_mesh_from_degree_elevation(self, linear_engine: "Engine"):
        """fh_set_mesh_from_degree_elevation: this engine's mesh becomes the degree elevation `linear_engine` holds, device to device"""
        self._adopt_held(self._lib.fh_set_mesh_from_degree_elevation, linear_engine, getattr(linear_engine, "_elevated", None))

    def _two_phase_u64(self, fn):
        n = C.c_uint64(0)
        self._check(fn(self._h, C.byref(n), None))
        out = np.zeros(int(n.value), dtype=np.uint64)
        if len(out):
            self._check(fn(self._h, C.byref(n), _ffi.up(out)))
        return out

    def boundary_vertices(self):
        """Mesh::find_boundary_vertices (mesh.rs:208-216): sorted, unique"""
        return self._two_phase_u64(self._lib.fh_boundary_vertices)

    def boundary_cells(self):
        """Mesh::find_boundary_cells (mesh.rs:154-163): sorted, unique"""
        return self._two_phase_u64(self._lib.fh_boundary_cells)

    def assemble_surface_load(self, out, load_kind, solution_dim, cells, local_faces, weights, points, data, data_count):
        """fh_assemble_surface_load(_dev): out += the traction / pressure load of the faces (cells, local_faces)"""
        w, p = _ffi.as_f64(weights), _ffi.as_f64(points)
        if _is_torch(out):
            import torch

            dev = out.device
            ct = cells if _is_torch(cells) else torch.from_numpy(np.ascontiguousarray(cells, dtype=np.uint64).view(np.int64)).to(dev)
            lt = local_faces if _is_torch(local_faces) else torch.from_numpy(np.ascontiguousarray(local_faces, dtype=np.uint32).view(np.int32)).to(dev)
            dt = data if _is_torch(data) else torch.from_numpy(_ffi.as_f64(data)).to(dev)
            self._check(self._lib.fh_assemble_surface_load_dev(self._h, load_kind, solution_dim, C.c_void_p(ct.data_ptr()), C.c_void_p(lt.data_ptr()),
                                                               ct.numel(), _ffi.fp(w), _ffi.fp(p), len(w), C.c_void_p(dt.data_ptr()), int(data_count),
                                                               C.c_void_p(out.data_ptr())))
            torch.cuda.synchronize(dev)  # the temporaries above are released on return
        else:
            cs, ls, d = _ffi.as_u64(cells), np.ascontiguousarray(local_faces, dtype=np.uint32), _ffi.as_f64(data)
            self._check(self._lib.fh_assemble_surface_load(self._h, load_kind, solution_dim, _ffi.up(cs), ls.ctypes.data_as(_ffi.u32p), len(cs),
                                                           _ffi.fp(w), _ffi.fp(p), len(w), _ffi.fp(d), int(data_count), _ffi.fp(out)))

    def physical_face_quadrature_points(self, cells, local_faces, points):
        """fh_physical_face_quadrature_points -> x (F, nq, d)"""
        cs, ls, p = _ffi.as_u64(cells), np.ascontiguousarray(local_faces, dtype=np.uint32), _ffi.as_f64(points)
        d = _ffi.ELEM_DIM[self._mesh.elem_kind]
        nq = p.size // max(d - 1, 1)
        x = np.zeros((len(cs), nq, d))
        self._check(self._lib.fh_physical_face_quadrature_points(self._h, _ffi.up(cs), ls.ctypes.data_as(_ffi.u32p), len(cs), _ffi.fp(p), nq,
                                                                 _ffi.fp(x)))
        return x

    def spmv(self, values_t, x_t, y_t):
        self._check(self._lib.fh_spmv_dev(self._h, C.c_void_p(values_t.data_ptr()), C.c_void_p(x_t.data_ptr()),
                                          C.c_void_p(y_t.data_ptr())))

    def cg_solve(self, values, b, x, preconditioner=1, rel_tol=1e-9, max_iter=0):
        """fh_cg_solve(_dev): x is the initial guess on entry and the solution on return; returns the iteration count.
        Raises CgSolveError (carrying the iteration count) like ConjugateGradient::solve_with_guess."""
        it = C.c_uint64(0)
        if _is_torch(values):
            rc = self._lib.fh_cg_solve_dev(self._h, C.c_void_p(values.data_ptr()), C.c_void_p(b.data_ptr()),
                                           C.c_void_p(x.data_ptr()), preconditioner, rel_tol, max_iter, C.byref(it))
        else:
            rc = self._lib.fh_cg_solve(self._h, _ffi.fp(values), _ffi.fp(b), _ffi.fp(x), preconditioner, rel_tol, max_iter,
                                       C.byref(it))
        if rc in (7, 8, 9):
            raise CgSolveError(rc, (self._lib.fh_last_error(self._h) or b"").decode(), int(it.value))
        self._check(rc)
        return int(it.value)

    def estimate_error_squared(self, which, solution_dim, u_h, exact):
        out = C.c_double()
        names = ("fh_estimate_L2_error_squared", "fh_estimate_H1_seminorm_error_squared")
        if _is_torch(u_h):
            fn = getattr(self._lib, names[which] + "_dev")
            rc = fn(self._h, solution_dim, C.c_void_p(u_h.data_ptr()), C.c_void_p(exact.data_ptr()), C.byref(out))
        else:
            fn = getattr(self._lib, names[which])
            rc = fn(self._h, solution_dim, _ffi.fp(np.ascontiguousarray(u_h, dtype=np.float64)),
                    _ffi.fp(np.ascontiguousarray(exact, dtype=np.float64)), C.byref(out))
        failed = C.c_uint64(0)
        self._check(rc, failed)
        return out.value

    def assemble_scalar(self):
        out, failed = C.c_double(), C.c_uint64(0)
        self._check(self._lib.fh_assemble_scalar(self._h, C.byref(out), C.byref(failed)), failed)
        return out.value

    def element_matrices(self, first, count):
        s, n = self.solution_dim(), _ffi.ELEM_NODES[self._mesh.elem_kind]
        ld = s * n
        out = np.zeros((count, ld, ld))
        self._check(self._lib.fh_assemble_element_matrices(self._h, first, count, _ffi.fp(out)))
        return out.transpose(0, 2, 1).copy()  # column-major blocks -> [e][row][col]

    def set_obstacles(self, obstacles):
        """the rigid obstacles of the penalty contact term (fenris_amd.contact: an Obstacles, a list of obstacles, or None to clear them)"""
        from .contact import set_obstacles

        set_obstacles(self, obstacles)

    def set_obstacle_time(self, t, t_lag=None):
        """the contact clock of obstacles that move along a path (fenris_amd.contact.ObstaclePath): they stand at d(t), and the friction slip
        is taken relative to their displacement since t_lag (None: t, no displacement).  A solver or tangent whose obstacles are bound
        (with_obstacles) keeps the clock: when it has to hand its obstacles to the engine again, because another object used the engine in
        between, the clock goes with them.  Engine.set_obstacles and with_obstacles return it to (0, 0); the time integrators drive it
        themselves"""
        from .contact import set_obstacle_time

        set_obstacle_time(self, t, t_lag)

    # matrix-free operator (FH_LAPLACE, FH_LINEAR_ELASTIC): no pattern, no values
    def set_operator_dirichlet_nodes(self, nodes):
        """the node set of the matrix-free routes (None: none); a DofSet (fenris_amd.dirichlet) goes to set_operator_dirichlet_dofs"""
        if isinstance(nodes, _dirichlet.DofSet):
            return self._set_operator_dirichlet_masks(nodes.nodes, nodes.masks)
        self._mf_bound = None   # (MatrixFreeOperator: no operator's nodes are bound any more)
        nodes = _ffi.as_u64(nodes if nodes is not None else [])
        self._check(self._lib.fh_set_operator_dirichlet_nodes(self._h, _ffi.up(nodes) if len(nodes) else None, len(nodes)))

    def set_operator_dirichlet_dofs(self, nodes, components):
        """single components of the listed nodes (fh_set_operator_dirichlet_dofs): components is an (n, S) boolean array or a sequence of
        component indices applied to every node; replaces the set, nodes None clears it"""
        if nodes is None:
            return self.set_operator_dirichlet_nodes(None)
        self._set_operator_dirichlet_masks(*_dirichlet.dof_masks(nodes, components))

    def _set_operator_dirichlet_masks(self, nodes, masks):
        self._mf_bound = None
        nodes, masks = _ffi.as_u64(nodes), np.ascontiguousarray(masks, dtype=np.uint8)
        n = len(nodes)
        self._check(self._lib.fh_set_operator_dirichlet_dofs(self._h, _ffi.up(nodes) if n else None, _u8p(masks) if n else None, n))

    def apply_operator_dev(self, x_t, y_t):
        self._check(self._lib.fh_apply_operator_dev(self._h, C.c_void_p(x_t.data_ptr()), C.c_void_p(y_t.data_ptr())))

    def operator_diagonal_dev(self, diag_t):
        self._check(self._lib.fh_operator_diagonal_dev(self._h, C.c_void_p(diag_t.data_ptr())))

    def cg_solve_matrix_free(self, b, x, preconditioner=1, rel_tol=1e-9, max_iter=0):
        """fh_cg_solve_matrix_free(_dev): cg_solve with the matrix-free operator"""
        return self._cg_solve_free("matrix_free", b, x, preconditioner, rel_tol, max_iter)

    # matrix-free tangent T(u) = dr/du at the engine's u (every material), on the operator's Dirichlet nodes
    def apply_tangent_dev(self, x_t, y_t):
        self._check(self._lib.fh_apply_tangent_dev(self._h, C.c_void_p(x_t.data_ptr()), C.c_void_p(y_t.data_ptr())))

    def tangent_diagonal_dev(self, diag_t):
        self._check(self._lib.fh_tangent_diagonal_dev(self._h, C.c_void_p(diag_t.data_ptr())))

    def cg_solve_tangent(self, b, x, preconditioner=1, rel_tol=1e-9, max_iter=0):
        """fh_cg_solve_tangent(_dev): cg_solve with the matrix-free tangent"""
        return self._cg_solve_free("tangent", b, x, preconditioner, rel_tol, max_iter)

    # the shifted map (alpha M + beta T(u)) x with the mass of the density set here (one for the mesh, or one per element)
    def set_mass_density(self, rho):
        rho = np.ascontiguousarray(np.atleast_1d(np.asarray(rho, dtype=np.float64)).ravel())
        self._check(self._lib.fh_set_mass_density(self._h, _ffi.fp(rho), len(rho)))

    # the per-element expansion (thermal strain, swelling, growth): one stress-free stretch theta_e > 0 per element, which strains the elastic
    # operators on every element-to-node route of this engine until it is changed, cleared or the mesh is set again
    def set_element_expansion(self, theta):
        """fh_set_element_expansion: one stretch for the mesh (a scalar) or one per element; None clears the field"""
        if theta is None:
            self._check(self._lib.fh_set_element_expansion(self._h, None, 0))
            return
        theta = np.ascontiguousarray(np.atleast_1d(np.asarray(theta, dtype=np.float64)).ravel())
        if len(theta) == 0:
            raise ValueError("set_element_expansion needs a stretch (None clears the field)")
        self._check(self._lib.fh_set_element_expansion(self._h, _ffi.fp(theta), len(theta)))

    def set_thermal_expansion(self, T, alpha, T_ref=0.0):
        """fh_set_thermal_expansion: theta_e = 1 + alpha_e (mean nodal temperature of the element - T_ref); T: one value per node, alpha: a
        scalar or one value per element"""
        T = np.ascontiguousarray(np.asarray(T, dtype=np.float64).ravel())
        if len(T) != self.num_nodes():
            raise ValueError("set_thermal_expansion needs one temperature per node")
        alpha = np.ascontiguousarray(np.atleast_1d(np.asarray(alpha, dtype=np.float64)).ravel())
        self._check(self._lib.fh_set_thermal_expansion(self._h, _ffi.fp(T), _ffi.fp(alpha), len(alpha), float(T_ref)))

    def element_expansion(self):
        """fh_element_expansion: the stretch of every element (FH_INVALID_STATE when none is set)"""
        out = np.zeros(self.num_elements())
        self._check(self._lib.fh_element_expansion(self._h, _ffi.fp(out)))
        return out

    def thermal_load(self):
        """fh_thermal_load: f_th = -r(0) of linear elasticity under the field in force (FH_UNSUPPORTED for any other operator)"""
        out = np.zeros(self.solution_dim() * self.num_nodes())
        self._check(self._lib.fh_thermal_load(self._h, _ffi.fp(out)))
        return out

    def apply_shifted_tangent_dev(self, alpha, beta, x_t, y_t):
        self._check(self._lib.fh_apply_shifted_tangent_dev(self._h, float(alpha), float(beta), C.c_void_p(x_t.data_ptr()),
                                                           C.c_void_p(y_t.data_ptr())))

    def shifted_tangent_diagonal_dev(self, alpha, beta, diag_t):
        self._check(self._lib.fh_shifted_tangent_diagonal_dev(self._h, float(alpha), float(beta), C.c_void_p(diag_t.data_ptr())))

    def cg_solve_shifted_tangent(self, alpha, beta, b, x, preconditioner=1, rel_tol=1e-9, max_iter=0):
        """fh_cg_solve_shifted_tangent(_dev): cg_solve with alpha M + beta T(u)"""
        it = C.c_uint64(0)
        if _is_torch(b):
            rc = self._lib.fh_cg_solve_shifted_tangent_dev(self._h, float(alpha), float(beta), C.c_void_p(b.data_ptr()), C.c_void_p(x.data_ptr()),
                                                           preconditioner, rel_tol, max_iter, C.byref(it))
        else:
            rc = self._lib.fh_cg_solve_shifted_tangent(self._h, float(alpha), float(beta), _ffi.fp(b), _ffi.fp(x), preconditioner, rel_tol,
                                                       max_iter, C.byref(it))
        if rc in (7, 8, 9):
            raise CgSolveError(rc, (self._lib.fh_last_error(self._h) or b"").decode(), int(it.value))
        self._check(rc)
        return int(it.value)

    def _cg_solve_free(self, which, b, x, preconditioner, rel_tol, max_iter):
        it = C.c_uint64(0)
        if _is_torch(b):
            rc = getattr(self._lib, f"fh_cg_solve_{which}_dev")(self._h, C.c_void_p(b.data_ptr()), C.c_void_p(x.data_ptr()), preconditioner,
                                                                rel_tol, max_iter, C.byref(it))
        else:
            rc = getattr(self._lib, f"fh_cg_solve_{which}")(self._h, _ffi.fp(b), _ffi.fp(x), preconditioner, rel_tol, max_iter, C.byref(it))
        if rc in (7, 8, 9):
            raise CgSolveError(rc, (self._lib.fh_last_error(self._h) or b"").decode(), int(it.value))
        self._check(rc)
        return int(it.value)

    def newton_solve(self, alpha, beta, f, u_ref, u, tolerance, max_iterations=0, line_search=1, preconditioner=1, linear_rel_tol=1e-8,
                     linear_max_iter=0):
        """fh_newton_solve(_dev) on the operator's Dirichlet nodes and the density set here: u is the guess on entry and the iterate on return
        (numpy array, or a device tensor with f and u_ref tensors too; f, u_ref may be None).  Returns (status, stats[4], norms[3]): the
        Newton codes 10-12 are returned, not raised (MatrixFreeNewton raises them); every other error raises."""
        stats = np.zeros(4, dtype=np.uint64)
        norms = np.zeros(3)
        args = (float(alpha), float(beta))
        tail = (float(tolerance), int(max_iterations), int(line_search), int(preconditioner), float(linear_rel_tol), int(linear_max_iter),
                _ffi.up(stats), _ffi.fp(norms))
        if _is_torch(u):
            rc = self._lib.fh_newton_solve_dev(self._h, *args, _ptr(f), _ptr(u_ref), C.c_void_p(u.data_ptr()), *tail)
        else:
            rc = self._lib.fh_newton_solve(self._h, *args, _ffi.fp(f), _ffi.fp(u_ref), _ffi.fp(u), *tail)
        if rc not in (_ffi.FH_NEWTON_MAX_ITERATIONS, _ffi.FH_NEWTON_JACOBIAN_ERROR, _ffi.FH_NEWTON_LINE_SEARCH_FAILED):
            self._check(rc)
        return rc, stats, norms

    # the block-vector layer of the eigensolver (fenris_amd.eigen): column-major blocks, column j of a block at data_ptr + j ld doubles
    def block_gram(self, n, p, s_t, lds, q, t_t, ldt):
        """fh_block_gram_dev: G = S^T T (p x q numpy array) for the device blocks S (n x p, ld lds) and T (n x q, ld ldt)"""
        g = np.zeros((max(int(p), 1), max(int(q), 1)))
        self._check(self._lib.fh_block_gram_dev(self._h, int(n), int(p), _ptr(s_t), int(lds), int(q), _ptr(t_t), int(ldt), _ffi.fp(g)))
        return g

    def block_combine(self, n, p, s_t, lds, c, y_t, ldy, accumulate=False):
        """fh_block_combine_dev: Y = S C (accumulate: Y += S C) with the host matrix c (p x q); Y may not overlap S"""
        c = _ffi.as_f64(c)
        self._check(self._lib.fh_block_combine_dev(self._h, int(n), int(p), _ptr(s_t), int(lds), int(c.shape[1]), _ffi.fp(c), _ptr(y_t), int(ldy),
                                                   int(bool(accumulate))))

    def dense_generalized_eigh(self, A, B):
        """fh_dense_generalized_eigh (host): (w ascending, C with C^T B C = I) of A c = w B c"""
        rc, w, cm = _ffi.dense_generalized_eigh(A, B)
        if rc != _ffi.FH_OK:
            raise FenrisError(rc, "fh_dense_generalized_eigh: B is not positive definite" if rc == _ffi.FH_EIG_BREAKDOWN else "bad argument")
        return w, cm

    def apply_dirichlet_csr_dev(self, values_t, nodes):
        nodes = _ffi.as_u64(nodes)
        self._check(self._lib.fh_apply_dirichlet_csr_dev(self._h, C.c_void_p(values_t.data_ptr()), _ffi.up(nodes), len(nodes)))

    def apply_dirichlet_rhs_dev(self, rhs_t, nodes):
        nodes = _ffi.as_u64(nodes)
        self._check(self._lib.fh_apply_dirichlet_rhs_dev(self._h, C.c_void_p(rhs_t.data_ptr()), _ffi.up(nodes), len(nodes)))

    def apply_dirichlet_dofs_csr_dev(self, values_t, nodes, masks):
        nodes, masks = _ffi.as_u64(nodes), np.ascontiguousarray(masks, dtype=np.uint8)
        self._check(self._lib.fh_apply_dirichlet_dofs_csr_dev(self._h, C.c_void_p(values_t.data_ptr()), _ffi.up(nodes), _u8p(masks), len(nodes)))

    def apply_dirichlet_dofs_rhs_dev(self, rhs_t, nodes, masks):
        nodes, masks = _ffi.as_u64(nodes), np.ascontiguousarray(masks, dtype=np.uint8)
        self._check(self._lib.fh_apply_dirichlet_dofs_rhs_dev(self._h, C.c_void_p(rhs_t.data_ptr()), _ffi.up(nodes), _u8p(masks), len(nodes)))


class CgSolveError(FenrisError):
    """SolveError of fenris-sparse/src/cg.rs:277-318 (kind + iterations so far)"""

    KINDS = {7: "MaxIterationsReached", 8: "IndefiniteOperator", 9: "IndefinitePreconditioner"}

    def __init__(self, code, message, num_iterations):
        super().__init__(code, message)
        self.kind = self.KINDS.get(code, "?")
        self.num_iterations = num_iterations


def _u8p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def _is_torch(x):
    return hasattr(x, "data_ptr") and hasattr(x, "device")


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# ------------------------------------------------------------------------------------------ tables
class UniformQuadratureTable:
    """src/assembly/local/quadrature_table.rs:213-298"""

    def __init__(self, points, weights, data=None):
        self.points = _ffi.as_f64(points)
        self.weights = _ffi.as_f64(weights)
        self.data = data  # nq x 2 (mu, lambda) or None

    @classmethod
    def from_points_and_weights(cls, points, weights):
        """NOTE the argument order (points, weights) -- a rule is (weights, points); quadrature_table.rs:232"""
        return cls(points, weights)

    @classmethod
    def from_quadrature(cls, rule):
        weights, points = rule
        return cls(points, weights)

    def with_uniform_data(self, data):
        """quadrature_table.rs:264-266"""
        pair = data.as_pair() if hasattr(data, "as_pair") else tuple(data)
        return UniformQuadratureTable(self.points, self.weights, np.tile(np.asarray(pair, dtype=np.float64), (len(self.weights), 1)))

    def with_data(self, data):
        """quadrature_table.rs:252-262: one Parameters value per quadrature point"""
        arr = np.array([d.as_pair() if hasattr(d, "as_pair") else tuple(d) for d in data], dtype=np.float64)
        assert arr.shape == (len(self.weights), 2)
        return UniformQuadratureTable(self.points, self.weights, arr)


class CompactQuadratureTable:
    """src/assembly/local/quadrature_table.rs:300-439 (``from_quadrature_rules_and_map``) for rules that share one
    set of points and weights and differ in their data: ``rule_data[r]`` holds one Parameters value per point (or a
    single value, repeated), ``element_to_rule_map[e]`` picks the rule of element e.  Piecewise material data."""

    def __init__(self, points, weights, rule_data, element_to_rule_map):
        self.points = _ffi.as_f64(points)
        self.weights = _ffi.as_f64(weights)
        nq = len(self.weights)
        rules = []
        for rd in rule_data:
            if hasattr(rd, "as_pair"):
                rd = [rd] * nq
            arr = np.array([d.as_pair() if hasattr(d, "as_pair") else tuple(d) for d in rd], dtype=np.float64)
            if arr.shape != (nq, 2):
                raise ValueError("every rule needs one data value per quadrature point")  # check_rules_consistency
            rules.append(arr)
        self.rule_params = np.ascontiguousarray(np.stack(rules))
        self.element_to_rule_map = _ffi.as_u64(element_to_rule_map)
        if len(self.element_to_rule_map) and int(self.element_to_rule_map.max()) >= len(rules):
            raise ValueError("Each rule index must correspond to a provided quadrature rule.")  # quadrature_table.rs:366-372
        self.data = self.rule_params[0]

    @classmethod
    def from_quadrature_rules_and_map(cls, points, weights, data, element_to_rule_map):
        return cls(points, weights, data, element_to_rule_map)


class _RuleSetTable:
    """Quadrature tables whose rules differ in their POINTS (GeneralQuadratureTable, and CompactQuadratureTable with
    different point sets; quadrature_table.rs:57-210, 300-439).  The device kernels stage one rule per launch, so the
    global assemblers walk the distinct rules: uniform table of rule r + the element mask of the elements that use it
    (fh_set_active_elements), accumulating into the same output.  Identical rules are merged."""

    def __init__(self, rules, element_to_rule_map):
        self.rules = rules  # list of (weights, points, data (nq, 2) or None)
        self.element_to_rule_map = _ffi.as_u64(element_to_rule_map)
        self.weights, self.points, self.data = rules[0]

    @staticmethod
    def _norm(points, weights, data):
        w, p = _ffi.as_f64(weights), _ffi.as_f64(points)
        if data is None:
            d = None
        else:
            d = np.array([x.as_pair() if hasattr(x, "as_pair") else tuple(x) for x in data], dtype=np.float64).reshape(len(w), 2)
        if len(p) != len(w):
            raise ValueError("Rules must have an equal number of points and weights.")  # check_rules_consistency
        return w, p, d

    @classmethod
    def build(cls, per_entry_rules, entry_of_element):
        """dedupe identical (points, weights, data) triples"""
        keys, rules, remap = {}, [], []
        for w, p, d in per_entry_rules:
            key = (w.tobytes(), p.tobytes(), None if d is None else d.tobytes())
            if key not in keys:
                keys[key] = len(rules)
                rules.append((w, p, d))
            remap.append(keys[key])
        remap = np.asarray(remap, dtype=np.uint64)
        return cls(rules, remap[np.asarray(entry_of_element, dtype=np.int64)])


class GeneralQuadratureTable(_RuleSetTable):
    """src/assembly/local/quadrature_table.rs:57-210: one rule (points, weights, data) per element"""

    @classmethod
    def from_points_and_weights(cls, points, weights):
        return cls.from_points_weights_and_data(points, weights, None)

    @classmethod
    def from_points_weights_and_data(cls, points, weights, data):
        n = len(weights)
        if len(points) != n or (data is not None and len(data) != n):
            raise ValueError("Quadrature point arrays must have the same number of rules.")
        rules = [cls._norm(points[e], weights[e], None if data is None else data[e]) for e in range(n)]
        return cls.build(rules, np.arange(n))


def compact_quadrature_table(points, weights, data, element_to_rule_map):
    """CompactQuadratureTable::from_quadrature_rules_and_map (quadrature_table.rs:357-383) for NestedVec inputs: rules
    that share points and weights take the single-launch device table (CompactQuadratureTable), anything else is walked
    rule by rule."""
    rules = [_RuleSetTable._norm(points[r], weights[r], None if data is None else data[r]) for r in range(len(weights))]
    emap = _ffi.as_u64(element_to_rule_map)
    if len(emap) and int(emap.max()) >= len(rules):
        raise ValueError("Each rule index must correspond to a provided quadrature rule.")
    same = all(np.array_equal(r[0], rules[0][0]) and np.array_equal(r[1], rules[0][1]) for r in rules)
    if same and all(r[2] is not None for r in rules):
        return CompactQuadratureTable(rules[0][1], rules[0][0], [r[2] for r in rules], emap)
    return _RuleSetTable.build(rules, emap)


@dataclass
class DisjointSubsetsColors:
    """Vec<DisjointSubsets> (fenris-paradis/src/lib.rs:171-181) flattened: elements of colour c are
    labels[color_offsets[c]:color_offsets[c+1]] in ascending order."""
    color_offsets: np.ndarray
    labels: np.ndarray

    def __len__(self):
        return len(self.color_offsets) - 1

    def color(self, c):
        return self.labels[int(self.color_offsets[c]): int(self.color_offsets[c + 1])]


class CsrMatrix:
    """nalgebra_sparse::CsrMatrix triple (row_offsets, col_indices, values); values may be numpy or a
    torch tensor on the engine's device."""

    def __init__(self, row_offsets, col_indices, values):
        self.row_offsets, self.col_indices, self.values = row_offsets, col_indices, values

    def nnz(self):
        return len(self.values)

    def nrows(self):
        return len(self.row_offsets) - 1

    def to_scipy(self):
        import scipy.sparse as sp

        v = self.values.cpu().numpy() if _is_torch(self.values) else self.values
        n = self.nrows()
        return sp.csr_matrix((v, self.col_indices.astype(np.int64), self.row_offsets.astype(np.int64)), shape=(n, n))


# ------------------------------------------------------------------------------------------ local
class ElementEllipticAssemblerBuilder:
    """src/assembly/local/elliptic.rs:63-150"""

    def __init__(self, engine: Optional[Engine] = None):
        self._engine, self._space, self._op, self._qtable, self._u, self._has_u = engine, None, None, None, None, False

    @classmethod
    def new(cls, engine: Optional[Engine] = None):
        return cls(engine)

    def with_finite_element_space(self, space: Mesh):
        self._space = space
        return self

    def with_operator(self, op):
        self._op = op
        return self

    def with_quadrature_table(self, qtable: UniformQuadratureTable):
        self._qtable = qtable
        return self

    def with_u(self, u):
        self._u, self._has_u = u, True
        return self

    def build(self) -> "ElementEllipticAssembler":
        if self._space is None or self._op is None or self._qtable is None or not self._has_u:
            raise ValueError("builder incomplete: space, operator, quadrature table and u are all required")
        return ElementEllipticAssembler(self._engine or Engine(), self._space, self._op, self._qtable, self._u)


class ElementEllipticAssembler(_Composable):
    """ElementEllipticAssembler<Mesh, Op, UniformQuadratureTable> (elliptic.rs:152-340), device resident."""

    def __init__(self, engine, space, op, qtable, u):
        self.engine, self.space, self.op, self.qtable = engine, space, op, qtable
        engine.set_mesh(space)
        engine.set_operator(op.op_kind)
        s = engine.solution_dim()
        if u is not None and not _is_torch(u):
            u = _ffi.as_f64(u)
            if len(u) != s * space.num_nodes():
                raise ValueError("Local element dofs (u) dimension mismatch")  # elliptic.rs:385-389
        engine.set_quadrature_table(qtable)
        if op.op_kind == _ffi.TENSOR:   # the operator's data: one tensor per point of the table just set
            engine.set_operator_tensor(op.tensors_for(len(qtable.weights), space.vertices.shape[1]), op.symmetric)
        engine.set_u(u)

    # ElementConnectivityAssembler (src/assembly/local.rs:18-47)
    def solution_dim(self):
        return self.engine.solution_dim()

    def num_elements(self):
        return self.engine.num_elements()

    def num_nodes(self):
        return self.engine.num_nodes()

    def element_node_count(self, _element_index):
        return _ffi.ELEM_NODES[self.space.elem_kind]

    def populate_element_nodes(self, output, element_index):
        output[:] = self.space.connectivity[element_index]

    # ElementMatrixAssembler::assemble_element_matrix_into (local.rs:78)
    def assemble_element_matrix(self, element_index):
        return self.engine.element_matrices(element_index, 1)[0]

    def with_u(self, u):
        self.engine.set_u(u)
        return self


class ElementMassAssembler(ElementEllipticAssembler):
    """ElementMassAssembler (src/assembly/local/mass.rs:48-160): ``with_solution_dim(s).with_space(mesh)
    .with_quadrature_table(table)`` where the table's data is ``Density`` per point.  s must be 1 or the geometry
    dimension.  Only the matrix form exists (ElementMatrixAssembler)."""

    def __init__(self, solution_dim, engine=None):
        self._sdim, self._engine0, self._space0, self._qt0 = solution_dim, engine, None, None

    @classmethod
    def with_solution_dim(cls, solution_dim, engine: Optional[Engine] = None):
        return cls(solution_dim, engine)

    def with_space(self, space: Mesh):
        self._space0 = space
        return self._maybe_build()

    def with_quadrature_table(self, qtable: "UniformQuadratureTable"):
        self._qt0 = qtable
        return self._maybe_build()

    def _maybe_build(self):
        if self._space0 is None or self._qt0 is None:
            return self
        d = _ffi.ELEM_DIM[self._space0.elem_kind]
        if self._sdim not in (1, d):
            raise ValueError("solution_dim must be 1 or the geometry dimension")
        if self._qt0.data is None:
            raise ValueError("the mass assembler needs a Density per quadrature point")

        class _Op:
            op_kind = _ffi.MASS_SCALAR if self._sdim == 1 else _ffi.MASS_VECTOR

        ElementEllipticAssembler.__init__(self, self._engine0 or Engine(), self._space0, _Op(), self._qt0, None)
        return self


class ElementSourceAssemblerBuilder:
    """src/assembly/local/source.rs:24-94"""

    def __init__(self, engine: Optional[Engine] = None):
        self._engine, self._space, self._source, self._qtable = engine, None, None, None

    @classmethod
    def new(cls, engine: Optional[Engine] = None):
        return cls(engine)

    def with_finite_element_space(self, space: Mesh):
        self._space = space
        return self

    def with_source(self, source):
        self._source = source
        return self

    def with_quadrature_table(self, qtable: "UniformQuadratureTable"):
        self._qtable = qtable
        return self

    def build(self) -> "ElementSourceAssembler":
        if self._space is None or self._source is None or self._qtable is None:
            raise ValueError("space, source and quadrature table are required")
        return ElementSourceAssembler(self._engine or Engine(), self._space, self._source, self._qtable)


class ElementSourceAssembler(_Composable):
    """src/assembly/local/source.rs:96-216: an ElementVectorAssembler for the (f, v) term.  ``source`` is a
    GravitySource (uniform Density table) or a SourceFunction (sampled on the host at the physical quadrature
    points, integrated on the device)."""

    def __init__(self, engine, space, source, qtable):
        self.engine, self.space, self.source, self.qtable = engine, space, source, qtable
        d = _ffi.ELEM_DIM[space.elem_kind]
        if source.solution_dim not in (1, d):
            raise ValueError("solution_dim must be 1 or the geometry dimension")
        engine.set_mesh(space)
        engine.set_quadrature_table(qtable)

    def solution_dim(self):
        return self.source.solution_dim

    def num_elements(self):
        return self.space.num_elements()

    def num_nodes(self):
        return self.space.num_nodes()

    def element_node_count(self, _element_index):
        return _ffi.ELEM_NODES[self.space.elem_kind]

    def populate_element_nodes(self, output, element_index):
        output[:] = self.space.connectivity[element_index]

    def assemble_vector_into_engine(self, output):
        s = self.source.solution_dim
        if hasattr(self.source, "gravitational_acceleration"):
            if self.qtable.data is None:
                raise ValueError("GravitySource needs a Density per quadrature point")
            self.engine.assemble_source_vector(output, s, g=self.source.gravitational_acceleration)
            return
        x = self.engine.physical_quadrature_points(len(self.qtable.weights))
        vals = np.ascontiguousarray(self.source.evaluate(x, self.qtable.data), dtype=np.float64)
        if vals.shape != (self.num_elements(), len(self.qtable.weights), s):
            raise ValueError("source values must have shape (E, nq, solution_dim)")
        if _is_torch(output):
            import torch

            vals_t = torch.from_numpy(vals).to(output.device)
            self.engine.assemble_source_vector(output, s, values=vals_t)
        else:
            self.engine.assemble_source_vector(output, s, values=vals)


class MockElementAssembler:
    """Generic ElementConnectivityAssembler with ragged node lists
    (tests/unit_tests/assembly/global.rs MockElementAssembler)."""

    def __init__(self, solution_dim, num_nodes, element_connectivities, engine: Optional[Engine] = None):
        self.engine = engine or Engine()
        offs = np.cumsum([0] + [len(c) for c in element_connectivities]).astype(np.uint64)
        nodes = np.array([x for c in element_connectivities for x in c], dtype=np.uint64)
        self.engine.set_connectivity_ragged(solution_dim, num_nodes, offs, nodes)


# ------------------------------------------------------------------------------------------ global
class CsrAssembler:
    """src/assembly/global.rs:24-183.  ``scatter`` picks the device strategy (default: atomic adds)."""

    def __init__(self, scatter=SCATTER_ATOMIC):
        self.scatter = scatter

    def assemble_pattern(self, element_assembler):
        """global.rs:65-120 -> (row_offsets, col_indices) as uint64 arrays"""
        if is_composed(element_assembler):
            return _compose.aggregate_pattern(element_assembler)
        return element_assembler.engine.pattern()

    def assemble(self, element_assembler, device_values=False):
        """global.rs:124-131"""
        if is_composed(element_assembler):  # AggregateElementAssembler / MapElementNodes / TransformElementMatrix
            import torch

            ro, ci = _compose.aggregate_pattern(element_assembler)
            values = torch.zeros(len(ci), dtype=torch.float64, device="cuda")
            _compose.assemble_matrix_into(ro, ci, values, element_assembler, self.scatter)
            return CsrMatrix(ro, ci, values if device_values else values.cpu().numpy())
        eng = element_assembler.engine
        ro, ci = eng.pattern()
        if device_values:
            import torch

            values = torch.zeros(len(ci), dtype=torch.float64, device=f"cuda:{eng.device}")
        else:
            values = np.zeros(len(ci))
        csr = CsrMatrix(ro, ci, values)
        self.assemble_into_csr(csr, element_assembler)
        return csr

    def assemble_into_csr(self, csr: CsrMatrix, element_assembler):
        """global.rs:133-182: accumulates into csr.values"""
        if is_composed(element_assembler):
            import torch

            on_dev = _is_torch(csr.values)
            values = csr.values if on_dev else torch.from_numpy(np.ascontiguousarray(csr.values)).cuda()
            _compose.assemble_matrix_into(csr.row_offsets, csr.col_indices, values, element_assembler, self.scatter)
            if not on_dev:
                csr.values[:] = values.cpu().numpy()
            return
        eng = element_assembler.engine
        if eng.nnz() == 0 and len(csr.values):
            eng.build_pattern()
        if len(csr.values) != eng.nnz():
            raise ValueError("CSR matrix does not have the pattern of this element assembler")
        flags = self.scatter

        if flags == SCATTER_COLORED:
            eng.color()
        eng.assemble_matrix(csr.values, flags)


class CsrParAssembler:
    """src/assembly/global.rs:185-377: colour-by-colour scatter without atomics."""

    def assemble_pattern(self, element_assembler):
        return element_assembler.engine.pattern()

    def assemble(self, colors: DisjointSubsetsColors, element_assembler):
        eng = element_assembler.engine
        ro, ci = eng.pattern()
        csr = CsrMatrix(ro, ci, np.zeros(len(ci)))
        self.assemble_into_csr(csr, colors, element_assembler)
        return csr

    def assemble_into_csr(self, csr: CsrMatrix, colors: DisjointSubsetsColors, element_assembler):
        eng = element_assembler.engine
        if len(csr.values) != eng.nnz():
            raise ValueError("CSR matrix does not have the pattern of this element assembler")
        eng.set_colors(colors)
        eng.assemble_matrix(csr.values, SCATTER_COLORED)


class VectorAssembler:
    """src/assembly/global.rs:569-616"""

    def assemble_vector(self, element_assembler):
        out = np.zeros(element_assembler.solution_dim() * element_assembler.num_nodes())
        self.assemble_vector_into(out, element_assembler)
        return out

    def assemble_vector_into(self, output, element_assembler):
        n = element_assembler.solution_dim() * element_assembler.num_nodes()
        if (output.numel() if _is_torch(output) else len(output)) != n:
            raise ValueError("Output dimensions mismatch")  # global.rs:592
        if is_composed(element_assembler):
            import torch

            on_dev = _is_torch(output)
            out_t = output if on_dev else torch.from_numpy(np.ascontiguousarray(output)).cuda()
            _compose.assemble_vector_into(out_t, element_assembler)
            if not on_dev:
                output[:] = out_t.cpu().numpy()
        elif hasattr(element_assembler, "assemble_vector_into_engine"):  # ElementSourceAssembler
            element_assembler.assemble_vector_into_engine(output)
        else:
            element_assembler.engine.assemble_vector(output)


class VectorParAssembler(VectorAssembler):
    """src/assembly/global.rs:618-686 (colours are not needed on the device: atomic adds)"""

    def assemble_vector(self, colors, element_assembler):  # noqa: D401 - signature of the reference
        return VectorAssembler.assemble_vector(self, element_assembler)


def assemble_scalar(element_assembler):
    """global.rs:697-711"""
    if is_composed(element_assembler):
        return _compose.assemble_scalar(element_assembler)
    return float(element_assembler.engine.assemble_scalar())


def color_nodes(mesh_or_assembler, engine: Optional[Engine] = None) -> DisjointSubsetsColors:
    """global.rs:540-551 + sequential_greedy_coloring (fenris-paradis/src/coloring.rs:6-70)"""
    if hasattr(mesh_or_assembler, "engine"):
        return mesh_or_assembler.engine.color()
    eng = engine or Engine()
    eng.set_mesh(mesh_or_assembler)
    return eng.color()


def apply_homogeneous_dirichlet_bc_csr(csr: CsrMatrix, nodes, solution_dim, element_assembler):
    """global.rs:379-451 on device-resident values"""
    assert solution_dim == element_assembler.solution_dim()
    eng = element_assembler.engine
    if _is_torch(csr.values):
        eng.apply_dirichlet_csr_dev(csr.values, nodes)
    else:
        import torch

        t = torch.from_numpy(csr.values).to(f"cuda:{eng.device}")
        eng.apply_dirichlet_csr_dev(t, nodes)
        csr.values[:] = t.cpu().numpy()


def apply_homogeneous_dirichlet_dofs_csr(csr: CsrMatrix, nodes, components, element_assembler):
    """apply_homogeneous_dirichlet_bc_csr for single components: the rows and columns of the listed dofs are zeroed inside their node
    blocks, their diagonal is the same scale.  components: an (n, S) boolean array or component indices applied to every node"""
    eng = element_assembler.engine
    nodes, masks = _dirichlet.dof_masks(nodes, components)
    if _is_torch(csr.values):
        eng.apply_dirichlet_dofs_csr_dev(csr.values, nodes, masks)
    else:
        import torch

        t = torch.from_numpy(csr.values).to(f"cuda:{eng.device}")
        eng.apply_dirichlet_dofs_csr_dev(t, nodes, masks)
        csr.values[:] = t.cpu().numpy()


def apply_homogeneous_dirichlet_dofs_rhs(rhs, nodes, components, element_assembler):
    """zeroes the listed dofs of rhs (a numpy array or a device tensor, in place)"""
    nodes, masks = _dirichlet.dof_masks(nodes, components)
    if _is_torch(rhs):
        element_assembler.engine.apply_dirichlet_dofs_rhs_dev(rhs, nodes, masks)
    else:
        rhs.reshape(-1)[_dirichlet.DofSet(nodes, masks).dof_indices(element_assembler.solution_dim())] = 0.0


def apply_homogeneous_dirichlet_bc_rhs(rhs, nodes, solution_dim):
    """global.rs:479-495 (host arrays: trivial)"""
    nodes = np.asarray(nodes, dtype=np.int64)
    for i in range(solution_dim):
        rhs[solution_dim * nodes + i] = 0.0


# ------------------------------------------------------------------------------------------ solve + error estimation
class RelativeResidualCriterion:
    """fenris-sparse/src/cg.rs:86-124: ||r|| <= tol ||b|| on CG's own residual (default 1e-8 for f64)"""

    def __init__(self, tol=1e-8):
        self.tol = float(tol)


class JacobiPreconditioner:
    """the inverse diagonal, built on the device (matrix.diagonal_as_csr() + recip, poisson_mms_common.rs:148-151)"""


class IdentityOperator:
    """fenris-sparse/src/cg.rs:54-61"""


class MatrixFreeOperator:
    """A LinearOperator (fenris-sparse/src/cg.rs:16-51) of an element assembler whose operator is linear (Laplace, LinearElastic):
    y = A x through the element pass of the residual, with neither pattern nor values.  With Dirichlet nodes, A is the matrix that
    apply_homogeneous_dirichlet_bc_csr leaves of the assembled one.  The nodes belong to this object: they are handed to the
    assembler's engine before every use, so several operators may share one assembler.  Vectors: numpy arrays or device tensors."""

    def __init__(self, element_assembler):
        self.element_assembler = element_assembler
        self.engine = element_assembler.engine
        self._nodes = None
        self._mg = None

    def with_dirichlet_nodes(self, nodes):
        self._nodes = None if nodes is None else _ffi.as_u64(nodes).copy()
        self._bind(force=True)
        return self

    def with_dirichlet_dofs(self, nodes, components):
        """single components of the listed nodes (rollers): components is an (n, S) boolean array or component indices applied to every
        node, so with_dirichlet_dofs(face_x0, [0]) holds u_x on that face.  Calls accumulate (with what with_dirichlet_nodes set, every
        component of those nodes); with_dirichlet_nodes starts over.  Returns self"""
        return _dirichlet.with_dirichlet_dofs(self, nodes, components)

    def with_multigrid(self, mg):
        """a GeometricMultigrid (fenris_amd.multigrid) over this operator's assembler: cg_solve then defaults to PRECOND_MULTIGRID"""
        self._mg = mg
        return self

    def _mg_density(self):
        return None

    def _bind(self, force=False):
        # (the engine keeps the nodes of the operator that used it last: handed over again only when another operator has used it since)
        if force or getattr(self.engine, "_mf_bound", None) is not self:
            self.engine.set_operator_dirichlet_nodes(self._nodes)
            self.engine._mf_bound = self
        _contact.bind_obstacles(self, force)

    def apply(self, y, x):
        """y = A x (y overwritten, like LinearOperator::apply)"""
        self._bind()
        if _is_torch(x):
            self._apply_dev(x, y)
            return y
        import torch

        xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(f"cuda:{self.engine.device}")
        yt = torch.empty_like(xt)
        self._apply_dev(xt, yt)
        y[...] = yt.cpu().numpy().reshape(np.shape(y))
        return y

    def diagonal(self, device=False):
        """the diagonal of A (numpy array, or a device tensor when device=True)"""
        import torch

        self._bind()
        n = self.element_assembler.solution_dim() * self.engine.num_nodes()
        d = torch.empty(n, dtype=torch.float64, device=f"cuda:{self.engine.device}")
        self._diagonal_dev(d)
        return d if device else d.cpu().numpy()

    def cg_solve(self, b, x, preconditioner=None, rel_tol=1e-9, max_iter=0):
        """fh_cg_solve_matrix_free(_dev) on this operator; returns the iteration count.  preconditioner None: PRECOND_MULTIGRID with a
        hierarchy (with_multigrid), else Jacobi"""
        self._bind()
        if preconditioner is None:
            preconditioner = _ffi.PRECOND_MULTIGRID if self._mg is not None else _ffi.PRECOND_JACOBI
        if preconditioner == _ffi.PRECOND_MULTIGRID and self._mg is not None:
            self._mg._bind(self._nodes, self._mg_density())
        return self._cg_solve(b, x, preconditioner, rel_tol, max_iter)

    def with_element_expansion(self, theta):
        """the per-element expansion of the engine (Engine.set_element_expansion: a scalar, one stretch per element, None to clear it).  The
        field belongs to the engine, not to this object: every object on the same engine sees it until it is changed; returns self"""
        self.engine.set_element_expansion(theta)
        return self

    def _apply_dev(self, x_t, y_t):
        self.engine.apply_operator_dev(x_t, y_t)

    def _diagonal_dev(self, d_t):
        self.engine.operator_diagonal_dev(d_t)

    def _cg_solve(self, b, x, preconditioner, rel_tol, max_iter):
        return self.engine.cg_solve_matrix_free(b, x, preconditioner, rel_tol, max_iter)


class MatrixFreeTangent(MatrixFreeOperator):
    """The tangent T(u) = dr/du of an element assembler's residual at its current u (any material: Laplace, LinearElastic, NeoHookean,
    StVK, StableNeoHookean), applied without pattern or values: the matrix assemble_matrix forms for the same u, without forming it.  The interface of
    MatrixFreeOperator (Dirichlet nodes owned by the object, apply on numpy arrays or device tensors, diagonal, cg_solve); its Jacobi
    preconditioner takes the tangent's diagonal.  Changing the assembler's u (with_u) changes the operator."""

    def with_obstacles(self, obstacles):
        """the rigid obstacles whose penalty term B(u) joins T(u) (fenris_amd.contact.Obstacles; None: none); they belong to this object"""
        return _contact.with_obstacles(self, obstacles)

    def with_friction_reference(self, ubar):
        """the lag displacement of the obstacles' friction term (fenris_amd.contact; a copy is kept); returns self"""
        return _contact.with_friction_reference(self, ubar)

    def _apply_dev(self, x_t, y_t):
        self.engine.apply_tangent_dev(x_t, y_t)

    def _diagonal_dev(self, d_t):
        self.engine.tangent_diagonal_dev(d_t)

    def _cg_solve(self, b, x, preconditioner, rel_tol, max_iter):
        return self.engine.cg_solve_tangent(b, x, preconditioner, rel_tol, max_iter)


class MatrixFreeShiftedTangent(MatrixFreeOperator):
    """alpha M + beta T(u) of an element assembler (Laplace, LinearElastic, NeoHookean, StVK, StableNeoHookean), the system of an implicit time step (backward
    Euler: alpha = 1, beta = dt^2), applied without pattern or values.  M is the mass matrix the assembled mass operator forms on the same
    mesh and quadrature table with this object's density (a scalar for the whole mesh, or one value per element), the scalar mass for
    Laplace and the vector mass for the materials; T(u) is MatrixFreeTangent's map at the assembler's current u.  Density, coefficients and
    Dirichlet nodes belong to this object and are handed to the engine before every use, so several such objects may share one assembler.
    The interface of MatrixFreeOperator (apply, diagonal, cg_solve; ConjugateGradient.with_operator accepts it)."""

    def __init__(self, element_assembler, density, alpha, beta):
        super().__init__(element_assembler)
        self._rho = np.ascontiguousarray(np.atleast_1d(np.asarray(density, dtype=np.float64)).ravel()).copy()
        self.alpha, self.beta = float(alpha), float(beta)
        self.engine.set_mass_density(self._rho)   # (checks the count now)
        self.engine._mass_bound = self

    def with_coefficients(self, alpha, beta):
        """new alpha, beta (e.g. another dt between steps); returns self"""
        self.alpha, self.beta = float(alpha), float(beta)
        return self

    def with_obstacles(self, obstacles):
        """the rigid obstacles whose penalty term joins the map: alpha M + beta (T(u) + B(u)) (None: none); they belong to this object"""
        return _contact.with_obstacles(self, obstacles)

    def with_friction_reference(self, ubar):
        """the lag displacement of the obstacles' friction term (fenris_amd.contact; a copy is kept); returns self"""
        return _contact.with_friction_reference(self, ubar)

    def _mg_density(self):
        return self._rho if self.alpha != 0.0 else None

    def _bind(self, force=False):
        super()._bind(force)
        if force or getattr(self.engine, "_mass_bound", None) is not self:
            self.engine.set_mass_density(self._rho)
            self.engine._mass_bound = self

    def _apply_dev(self, x_t, y_t):
        self.engine.apply_shifted_tangent_dev(self.alpha, self.beta, x_t, y_t)

    def _diagonal_dev(self, d_t):
        self.engine.shifted_tangent_diagonal_dev(self.alpha, self.beta, d_t)

    def _cg_solve(self, b, x, preconditioner, rel_tol, max_iter):
        return self.engine.cg_solve_shifted_tangent(self.alpha, self.beta, b, x, preconditioner, rel_tol, max_iter)


class MatrixFreeMass(MatrixFreeShiftedTangent):
    """The mass matrix M of MatrixFreeShiftedTangent alone (alpha = 1, beta = 0: u is not read), plus its row-sum lumping."""

    def __init__(self, element_assembler, density):
        super().__init__(element_assembler, density, 1.0, 0.0)

    def with_element_expansion(self, theta):
        """the mass is that of the reference volume and does not see the expansion: set the field on an object that does"""
        raise ValueError("MatrixFreeMass ignores the element expansion; set it on the engine or on a tangent, solver or integrator")

    def lumped(self, device=False):
        """M 1 without Dirichlet rows: the row-sum lumped mass for explicit stepping, in one application.  As for any row-sum lumping, some
        entries can be zero or negative on quadratic kinds (the vertex rows of Tet10 and Tri6, for example)."""
        import torch

        saved = self._nodes
        self._nodes = None
        self._bind(force=True)
        try:
            n = self.element_assembler.solution_dim() * self.engine.num_nodes()
            dev = f"cuda:{self.engine.device}"
            ones = torch.ones(n, dtype=torch.float64, device=dev)
            y = torch.empty_like(ones)
            self.engine.apply_shifted_tangent_dev(1.0, 0.0, ones, y)
        finally:
            self._nodes = saved
            self._bind(force=True)
        return y if device else y.cpu().numpy()


# ------------------------------------------------------------------------------------------ Newton (fenris-optimize/src/newton.rs)
@dataclass
class NewtonSettings:
    """NewtonSettings { max_iterations, tolerance } (newton.rs:20-24): converged when ||F||_2 <= tolerance; max_iterations None: no limit"""

    max_iterations: Optional[int] = None
    tolerance: float = 1e-8


class NoLineSearch:
    """the full Newton step (newton.rs:140-163)"""

    kind = _ffi.NEWTON_NO_LINE_SEARCH


class BacktrackingLineSearch:
    """Armijo backtracking with c = 1e-4 and step lengths 1, 0.75, 0.5, 0.25, 0.0625, ... down to 1e-6 (newton.rs:165-249)"""

    kind = _ffi.NEWTON_BACKTRACKING


@dataclass
class NewtonResult:
    """what fh_newton_solve reports: Newton iterations, residual evaluations, PCG iterations summed, the last PCG's status, ||F(u_0)||,
    ||F|| at return and the last accepted step length (0: none)"""

    iterations: int
    residual_evaluations: int
    linear_iterations: int
    linear_status: int
    initial_residual_norm: float
    residual_norm: float
    step_length: float


class NewtonError(FenrisError):
    """NewtonError (newton.rs:25-34); `result` holds the NewtonResult of the failed solve, whose u is the reference's x at the failure"""

    def __init__(self, code, message, result):
        super().__init__(code, message)
        self.result = result


class MaximumIterationsReached(NewtonError):
    """NewtonError::MaximumIterationsReached(iterations)"""

    @property
    def iterations(self):
        return self.result.iterations


class JacobianError(NewtonError):
    """NewtonError::JacobianError: the inner PCG failed; cg_code is its status (7-9, see CgSolveError)"""

    @property
    def cg_code(self):
        return self.result.linear_status


class LineSearchError(NewtonError):
    """NewtonError::LineSearchError: no step length above 1e-6 passed, or (a deviation from newton.rs) an accepted state's ||F|| is not finite"""


class MatrixFreeNewton:
    """newton_line_search (fenris-optimize/src/newton.rs:77-130) on the device for F(u) = alpha M (u - u_ref) + beta (r(u) - f), r the
    element assembler's residual and M the mass of MatrixFreeShiftedTangent; the Jacobian is alpha M + beta T(u) and each Newton step is a
    matrix-free Jacobi-PCG solve on it.  Static equilibrium (alpha = 0, beta = 1) or a backward-Euler step (with_inertia(rho, 1, dt^2, u_ref)).
    Dirichlet nodes, load, density and coefficients belong to this object and are handed to the engine before every solve.  The assembler's
    u is the solution afterwards."""

    def __init__(self, element_assembler):
        self.element_assembler = element_assembler
        self.engine = element_assembler.engine
        self._nodes, self._f, self._u_ref, self._rho = None, None, None, None
        self.alpha, self.beta = 0.0, 1.0
        self._mg = None

    def with_multigrid(self, mg):
        """a GeometricMultigrid (fenris_amd.multigrid) over this assembler: solve then defaults to PRECOND_MULTIGRID; returns self"""
        self._mg = mg
        return self

    def with_dirichlet_nodes(self, nodes):
        """the nodes held at the values u has on entry to solve (None: none); returns self"""
        self._nodes = None if nodes is None else _ffi.as_u64(nodes).copy()
        self._bind(force=True)
        return self

    def with_dirichlet_dofs(self, nodes, components):
        """single components held at the values u has on entry to solve (MatrixFreeOperator.with_dirichlet_dofs); calls accumulate; returns self"""
        return _dirichlet.with_dirichlet_dofs(self, nodes, components)

    def with_load(self, f):
        """the load f of r(u) = f (numpy array or device tensor; None: zero); returns self"""
        self._f = f
        return self

    def with_inertia(self, density, alpha, beta, u_ref=None):
        """density (one value or one per element), coefficients and u_ref (None: zero) of the mass term; returns self"""
        self._rho = np.ascontiguousarray(np.atleast_1d(np.asarray(density, dtype=np.float64)).ravel()).copy()
        self.alpha, self.beta, self._u_ref = float(alpha), float(beta), u_ref
        self.engine.set_mass_density(self._rho)   # (checks the count now)
        self.engine._mass_bound = self
        return self

    def with_coefficients(self, alpha, beta):
        self.alpha, self.beta = float(alpha), float(beta)
        return self

    def _bind(self, force=False):
        # (the engine keeps the Dirichlet nodes and the density of the object that used it last, as for MatrixFreeOperator)
        if force or getattr(self.engine, "_mf_bound", None) is not self:
            self.engine.set_operator_dirichlet_nodes(self._nodes)
            self.engine._mf_bound = self
        if self._rho is not None and (force or getattr(self.engine, "_mass_bound", None) is not self):
            self.engine.set_mass_density(self._rho)
            self.engine._mass_bound = self
        _contact.bind_obstacles(self, force)

    def with_element_expansion(self, theta):
        """the per-element expansion of the engine (Engine.set_element_expansion: a scalar, one stretch per element, None to clear it).  The
        field belongs to the engine, not to this object: every object on the same engine sees it until it is changed; returns self"""
        self.engine.set_element_expansion(theta)
        return self

    def with_obstacles(self, obstacles):
        """the rigid obstacles of the penalty contact term: F = alpha M (u - u_ref) + beta (r(u) + g(u) - f) (None: none); returns self"""
        return _contact.with_obstacles(self, obstacles)

    def with_friction_reference(self, ubar):
        """the lag displacement of the obstacles' friction term: F = alpha M (u - u_ref) + beta (r + g + q - f) with normal force and
        tangent plane frozen at ubar (copied); a quasi-static user moves it to the converged u between load steps; returns self"""
        return _contact.with_friction_reference(self, ubar)

    def solve(self, u, settings: NewtonSettings = NewtonSettings(), line_search=None, preconditioner=None, linear_rel_tol=1e-8, linear_max_iter=0):
        """u: the guess with the Dirichlet values (numpy array or device tensor), overwritten by the solution.  Returns a NewtonResult;
        raises MaximumIterationsReached, JacobianError or LineSearchError with u holding the reference's x at the failure.  preconditioner
        None: PRECOND_MULTIGRID with a hierarchy (with_multigrid), else Jacobi."""
        self._bind()
        if preconditioner is None:
            preconditioner = _ffi.PRECOND_MULTIGRID if self._mg is not None else _ffi.PRECOND_JACOBI
        if preconditioner == _ffi.PRECOND_MULTIGRID and self._mg is not None:
            self._mg._bind(self._nodes, self._rho if self.alpha != 0.0 else None)
        ls = BacktrackingLineSearch() if line_search is None else line_search
        f, u_ref = self._f, self._u_ref
        n = self.element_assembler.solution_dim() * self.engine.num_nodes()
        if _is_torch(u):
            import torch

            # (written in place through its pointer: exactly n contiguous doubles on the engine's device)
            if u.dtype != torch.float64 or not u.is_contiguous() or u.numel() != n or u.device != torch.device(f"cuda:{self.engine.device}"):
                raise ValueError(f"u must be a contiguous float64 tensor of {n} entries on cuda:{self.engine.device}")
            dev = u.device
            f = None if f is None else torch.as_tensor(f, dtype=torch.float64).to(dev).reshape(-1).contiguous()
            u_ref = None if u_ref is None else torch.as_tensor(u_ref, dtype=torch.float64).to(dev).reshape(-1).contiguous()
            uu = u
        else:
            if np.size(u) != n:
                raise ValueError(f"u must hold {n} entries")
            f = None if f is None else _ffi.as_f64(f.cpu().numpy() if _is_torch(f) else f).reshape(-1)
            u_ref = None if u_ref is None else _ffi.as_f64(u_ref.cpu().numpy() if _is_torch(u_ref) else u_ref).reshape(-1)
            uu = _ffi.as_f64(u).reshape(-1)
        for name, v in (("f", f), ("u_ref", u_ref)):
            if v is not None and (v.numel() if _is_torch(v) else v.size) != n:
                raise ValueError(f"{name} must hold {n} entries")
        rc, st, nm = self.engine.newton_solve(self.alpha, self.beta, f, u_ref, uu, settings.tolerance, settings.max_iterations or 0, ls.kind,
                                              preconditioner, linear_rel_tol, linear_max_iter)
        if not _is_torch(u) and not np.shares_memory(uu, u):
            u[...] = uu.reshape(np.shape(u))
        res = NewtonResult(int(st[0]), int(st[1]), int(st[2]), int(st[3]), float(nm[0]), float(nm[1]), float(nm[2]))
        if rc != _ffi.FH_OK:
            cls = {_ffi.FH_NEWTON_MAX_ITERATIONS: MaximumIterationsReached, _ffi.FH_NEWTON_JACOBIAN_ERROR: JacobianError}.get(rc, LineSearchError)
            raise cls(rc, self.engine.last_error(), res)
        return res


class ConjugateGradient:
    """fenris-sparse/src/cg.rs:196-478, builder style.  The operator is the CSR matrix assembled by an element
    assembler of this package (its engine holds the pattern); values, right-hand side and solution may be numpy
    arrays or device tensors (all of one kind)."""

    def __init__(self):
        self._csr, self._asm, self._pre, self._crit, self._max_iter = None, None, IdentityOperator(), None, 0

    @classmethod
    def new(cls):
        return cls()

    def with_operator(self, csr, element_assembler=None):
        """(csr, element_assembler): the assembled matrix; or one MatrixFreeOperator / MatrixFreeTangent / MatrixFreeShiftedTangent"""
        if isinstance(csr, MatrixFreeOperator):
            self._csr, self._asm = csr, csr.element_assembler
        else:
            self._csr, self._asm = csr, element_assembler
        return self

    def with_preconditioner(self, preconditioner):
        self._pre = preconditioner
        return self

    def with_max_iter(self, max_iter):
        self._max_iter = int(max_iter)
        return self

    def with_stopping_criterion(self, criterion: RelativeResidualCriterion):
        self._crit = criterion
        return self

    def solve_with_guess(self, b, x):
        """x: initial guess, overwritten by the solution; returns CgOutput.num_iterations"""
        if self._csr is None or self._crit is None:
            raise ValueError("operator and stopping criterion are required")
        pre = 1 if isinstance(self._pre, JacobiPreconditioner) else 0
        from .amg import SmoothedAggregationAMG

        if isinstance(self._pre, SmoothedAggregationAMG):   # FH_PRECOND_AMG on the assembled matrix
            self._pre._attach()
            pre = _ffi.PRECOND_AMG
        if isinstance(self._csr, MatrixFreeOperator):   # Jacobi: the matrix-free diagonal (of the tangent for a MatrixFreeTangent)
            return self._csr.cg_solve(b, x, pre, self._crit.tol, self._max_iter)
        return self._asm.engine.cg_solve(self._csr.values, b, x, pre, self._crit.tol, self._max_iter)


def _sample(space_assembler, fn, nq):
    x = space_assembler.engine.physical_quadrature_points(nq)
    return np.ascontiguousarray(fn(x), dtype=np.float64)


def estimate_L2_error_squared(element_assembler, u, u_h, solution_dim=None):
    """src/error.rs:287-311.  ``u(x)`` is vectorised: (E, nq, d) physical points -> (E, nq, s) values."""
    s = solution_dim or element_assembler.solution_dim()
    nq = len(element_assembler.qtable.weights)
    return element_assembler.engine.estimate_error_squared(0, s, u_h, _sample(element_assembler, u, nq))


def estimate_L2_error(element_assembler, u, u_h, solution_dim=None):
    """src/error.rs:313-328"""
    return float(np.sqrt(estimate_L2_error_squared(element_assembler, u, u_h, solution_dim)))


def estimate_H1_seminorm_error_squared(element_assembler, u_grad, u_h, solution_dim=None):
    """src/error.rs:330-354.  ``u_grad(x)``: (E, nq, d) points -> (E, nq, d, s) with [i][k] = d u_k / d x_i."""
    s = solution_dim or element_assembler.solution_dim()
    nq = len(element_assembler.qtable.weights)
    return element_assembler.engine.estimate_error_squared(1, s, u_h, _sample(element_assembler, u_grad, nq))


def estimate_H1_seminorm_error(element_assembler, u_grad, u_h, solution_dim=None):
    """src/error.rs:356-372"""
    return float(np.sqrt(estimate_H1_seminorm_error_squared(element_assembler, u_grad, u_h, solution_dim)))
