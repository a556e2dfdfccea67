"""A reused context must answer like a fresh one.

A context (fh_ctx) carries several dozen cached tables, each kept valid by a generation counter or by a line in a setter.  Every test here
drives ONE long-lived engine through a script of setter calls (with assemblies in between, so that every cache is filled before the next
setter has to drop it), then builds a fresh engine that is given only the final state, and compares what the two compute route by route:
bit for bit against each other, and within 1e-12 max|want| against the CPU oracle (the pattern exactly).  Stale state that agrees between
the two engines cannot exist -- the fresh one has none --, and the oracle guards against a defect both share.  Bit for bit holds wherever
the library promises it: every kernel but the documented hardware-order ones (HARDWARE_ORDER below, with the measurement), for which the
reproducible form of the same route carries the bitwise check.  No route had to be exempted for a kernel choice that depends on the
context's history: the reused and the fresh engine name the same kernel on every route of every script.

The handle tests make a small AMG or multigrid hierarchy, solve once, change the mesh or the pattern under it and expect FH_INVALID_STATE
with a message naming the creating call: the hierarchies hold device pointers and sizes of the context they were made for (the lifetime
rule of include/fenris_hip.h).  They reach only those guards, never the stale memory behind them.

Finding on fh_set_connectivity_ragged (read in engine.hip, not provoked): it kept has_mask, user_mask, rs.active, nq, has_u and topo_gen of
the flat mesh before it.  With a mask left over, fh_pattern ended in build_compute_adjacency with ei.n == 0 (an element index k / 0) and an
`active` array of the old element count: an out-of-bounds read that the C ABI and Engine.set_connectivity_ragged could reach.  The ragged
setter now drops the per-mesh state the flat one drops; test_ragged_connectivity_between_flat_meshes walks that path."""
import ctypes as C

import numpy as np
import pytest

import fenris_amd as fa
from fenris_amd import _ffi, quadrature
from fenris_amd.assembly import _RuleSetTable
from fenris_amd.contact import HalfSpace
from fenris_amd.interpolate import SpatiallyIndexed

pytestmark = pytest.mark.gpu

FH_OK, FH_INVALID_STATE = 0, 5
LAME = (3.0e2, 5.0e2)
OPS = {"LAPLACE": _ffi.LAPLACE, "LINEAR_ELASTIC": _ffi.LINEAR_ELASTIC, "NEO_HOOKEAN": _ffi.NEO_HOOKEAN,
       "STABLE_NEO_HOOKEAN": _ffi.STABLE_NEO_HOOKEAN, "TENSOR": _ffi.TENSOR}
SCATTERS = (("gather", fa.SCATTER_GATHER), ("gather_reproducible", fa.SCATTER_GATHER | _ffi.ASSEMBLE_REPRODUCIBLE),
            ("atomic", fa.SCATTER_ATOMIC), ("colored", fa.SCATTER_COLORED))
# Kernels that add in hardware order, as include/fenris_hip.h documents under FH_ASSEMBLE_REPRODUCIBLE and engine_vector.hip at the residual's
# last resort: fp64 atomics on HBM (atomic scatter, the one-pass residual of the high-order kinds) or in LDS (the one-pass gather kernels).
# Two FRESH engines differ in the last bit there (measured: 367 of 105 336 values of k_gather_pipelined on the 9 x 7 x 6 box, 9 of 525
# entries of k_assemble_vector on Hex27), so a bitwise comparison says nothing about reuse.  Where BOTH engines name such a kernel for a
# route, its arrays are held to the oracle only; the kernel names are still compared, and the gather route is compared bit for bit in its
# reproducible form (values.gather_reproducible.*), which the same tables serve.
HARDWARE_ORDER = {"k_assemble_matrix<atomic>", "k_gather_pipelined", "k_assemble_matrix<gather>", "k_assemble_vector", "k_assemble_vector_stream"}
# Routes that launch nothing when the context holds their result (the boundary faces are kept across vertex updates, operators and masks; point
# location names no kernel of its own): last_kernel_name() there is the previous route's, which is a statement about the order of calls
NO_KERNEL_OF_THEIR_OWN = {"boundary.faces", "points.locate"}
GRAVITY = np.array([0.3, -9.81, 1.7])
RHO = 2.5
OBSERVE = "observe"   # a script step: run every route on the long-lived engine, so that its caches are full when the next setter arrives


def _rule(kind):
    return {fa.HEX8: lambda: quadrature.tensor.hexahedron_gauss(2), fa.HEX27: lambda: quadrature.tensor.hexahedron_gauss(3),
            fa.QUAD4: lambda: quadrature.tensor.quadrilateral_gauss(2), fa.TET4: lambda: quadrature.total_order.tetrahedron(2)}[kind]()


def _box(nx, ny, nz, jitter=0.0, seed=0):
    m = fa.procedural.create_rectangular_uniform_hex_mesh(1.0, nx, ny, nz, 1)
    if jitter:
        rng = np.random.default_rng(seed)
        m = fa.Mesh(m.vertices + jitter * rng.uniform(-1, 1, m.vertices.shape), m.connectivity, m.elem_kind)
    return m


def _permuted(mesh, seed):
    rng = np.random.default_rng(seed)
    vp = rng.permutation(mesh.num_nodes())
    inv = np.empty_like(vp)
    inv[vp] = np.arange(len(vp))
    conn = inv[np.asarray(mesh.connectivity).astype(np.int64)][rng.permutation(mesh.num_elements())]
    return fa.Mesh(mesh.vertices[vp], conn.astype(np.uint64), mesh.elem_kind)


def _sdim(op, d):
    return 1 if op == "LAPLACE" else d


def _u(mesh, op, seed):
    return 0.004 * np.random.default_rng(seed).standard_normal(_sdim(op, mesh.vertices.shape[1]) * mesh.num_nodes())


# ------------------------------------------------------------------------------------------ the state a script leaves, and its setters
class State:
    """what the documented semantics of the setters leave on a context: the fresh engine is built from this alone"""

    def __init__(self):
        self.mesh, self.op, self.tol, self.stream = None, None, None, None
        self._per_mesh()

    def _per_mesh(self):
        # fh_set_mesh drops: the quadrature table, u, the mask, the row range, the Dirichlet nodes, the density, the obstacles, the tensor
        self.rule = self.rules = self.u = self.mask = self.rows = self.dirichlet = self.density = self.obstacles = self.tensor = None

    def sdim(self):
        return _sdim(self.op, self.mesh.vertices.shape[1])


def set_mesh(mesh):
    def step(eng, st):
        eng.set_mesh(mesh)
        st.mesh = mesh
        st._per_mesh()
    return step


def set_op(op):
    def step(eng, st):
        old = st.sdim() if (st.op and st.mesh) else None
        eng.set_operator(OPS[op])
        st.op = op
        if st.mesh is not None and old is not None and st.sdim() != old:
            st.u = None   # another solution dim drops u
    return step


def _params(w):
    return np.tile(np.asarray(LAME), (len(w), 1))


def set_rule(w, p):
    def step(eng, st):
        eng.set_quadrature_uniform(w, p, _params(w))
        st.rule, st.rules = (w, p), None
    return step


def set_rules(groups, emap):
    """a rule-set table: groups = [(w, p), ...] with different points, emap[e] = the group of element e"""
    def step(eng, st):
        table = _RuleSetTable.build([(_ffi.as_f64(w), _ffi.as_f64(p), _params(w)) for w, p in groups], emap)
        eng.set_quadrature_table(table)
        st.rules, st.rule = (groups, np.asarray(emap)), None
    return step


def set_tensor(A, symmetric=False):
    def step(eng, st):
        eng.set_operator_tensor(A.reshape(A.shape[0], -1), symmetric)
        st.tensor = (A, symmetric)
    return step


def _setter(method, field):
    def make(value):
        def step(eng, st):
            getattr(eng, method)(value)
            setattr(st, field, value)
        return step
    return make


set_u = _setter("set_u", "u")
set_mask = _setter("set_active_elements", "mask")
set_tol = _setter("set_affine_tolerance", "tol")
set_dirichlet = _setter("set_operator_dirichlet_nodes", "dirichlet")
set_density = _setter("set_mass_density", "density")
set_obstacles = _setter("set_obstacles", "obstacles")


def set_rows(lo, hi):
    def step(eng, st):
        eng.set_row_range(lo, hi)
        st.rows = (lo, hi)
    return step


def update_vertices(v):
    def step(eng, st):
        eng.update_vertices(v)
        st.mesh = fa.Mesh(v, st.mesh.connectivity, st.mesh.elem_kind)
    return step


def set_stream(stream):
    def step(eng, st):
        eng._check(eng._lib.fh_set_stream(eng._h, C.c_void_p(stream.cuda_stream)))
        st.stream = stream
    return step


def problem(mesh, op, seed):
    """mesh + operator + the kind's rule + a u: the steps of a whole new problem on the context"""
    w, p = _rule(mesh.elem_kind)
    return [set_mesh(mesh), set_op(op), set_rule(w, p), set_u(_u(mesh, op, seed))]


def build(eng, st):
    """the final state on a fresh engine, each setter once"""
    if st.stream is not None:
        set_stream(st.stream)(eng, State())
    if st.tol is not None:
        eng.set_affine_tolerance(st.tol)
    eng.set_mesh(st.mesh)
    eng.set_operator(OPS[st.op])
    scratch = State()
    if st.rule is not None:
        set_rule(*st.rule)(eng, scratch)
    if st.rules is not None:
        set_rules(*st.rules)(eng, scratch)
    if st.tensor is not None:
        set_tensor(*st.tensor)(eng, scratch)
    for method, value in (("set_u", st.u), ("set_active_elements", st.mask), ("set_operator_dirichlet_nodes", st.dirichlet),
                          ("set_mass_density", st.density), ("set_obstacles", st.obstacles)):
        if value is not None:
            getattr(eng, method)(value)
    if st.rows is not None:
        eng.set_row_range(*st.rows)


# ------------------------------------------------------------------------------------------ observe: every route that owns a cache
def observe(eng, st, final=True):
    """{route: host array, or ("error", code) where the library refuses the route in this state}, {route: last_kernel_name()}.  Every route
    runs with the state as the script left it; the two toggles at the end (Dirichlet nodes, a density) are setter calls of their own and are
    taken back, so that they only run where both engines run them (final=True)."""
    import torch

    dev = f"cuda:{eng.device}"
    out, names = {}, {}
    n = st.sdim() * st.mesh.num_nodes()
    d = st.mesh.vertices.shape[1]

    def route(key, fn):
        try:
            out[key] = fn()
        except _ffi.FenrisError as e:
            if e.code in (_ffi.FH_HIP_ERROR, _ffi.FH_OUT_OF_MEMORY):
                pytest.exit(f"device error on route {key}: {e}", returncode=3)   # nothing more is started on a device that reported one
            out[key] = ("error", e.code)
        names[key] = eng.last_kernel_name()

    ro, ci = eng.pattern()
    out["pattern.row_offsets"], out["pattern.col_indices"] = ro, ci
    nnz = len(ci)

    def matrix(flags, fill):
        def run():
            v = np.full(nnz, fill)
            try:
                eng.assemble_matrix(v, flags)
            except _ffi.FenrisError as e:
                if e.code != FH_INVALID_STATE or (flags & 0xff) != fa.SCATTER_COLORED:
                    raise
                eng.color()   # (no colours yet for this mesh: they are kept across masks, operators and vertex updates, so made only here)
                eng.assemble_matrix(v, flags)
            return v
        return run

    for tag, flags in SCATTERS:
        route(f"values.{tag}.accumulate", matrix(flags, 0.0))
        route(f"values.{tag}.overwrite", matrix(flags | fa.ASSEMBLE_OVERWRITE, 7.0))

    def residual():
        r = np.zeros(n)
        eng.assemble_vector(r)
        return r

    def source():
        f = np.zeros(n)
        eng.assemble_source_vector(f, st.sdim(), g=GRAVITY[:st.sdim()])
        return f

    route("residual", residual)
    route("energy", lambda: np.array([eng.assemble_scalar()]))
    route("source", source)

    x = torch.from_numpy(np.cos(0.37 * np.arange(n))).to(dev)

    def device_vector(call):
        def run():
            y = torch.full((n,), 3.0, dtype=torch.float64, device=dev)
            torch.cuda.synchronize()
            call(y)
            eng.synchronize()
            return y.cpu().numpy()
        return run

    def matrix_free(tag):
        route(f"mf.apply.{tag}", device_vector(lambda y: eng.apply_operator_dev(x, y)))
        route(f"mf.diagonal.{tag}", device_vector(lambda y: eng.operator_diagonal_dev(y)))
        route(f"mf.tangent.{tag}", device_vector(lambda y: eng.apply_tangent_dev(x, y)))
        route(f"mf.tangent_diagonal.{tag}", device_vector(lambda y: eng.tangent_diagonal_dev(y)))

    def shifted(tag):
        route(f"mf.shifted.{tag}", device_vector(lambda y: eng.apply_shifted_tangent_dev(1.5, 0.25, x, y)))
        route(f"mf.shifted_diagonal.{tag}", device_vector(lambda y: eng.shifted_tangent_diagonal_dev(1.5, 0.25, y)))

    matrix_free("state")
    shifted("state")
    route("boundary.faces", lambda: np.concatenate([a.astype(np.float64).ravel() for a in eng.find_boundary_faces()]))
    pts = st.mesh.vertices.min(axis=0) + np.random.default_rng(50).random((50, d)) * np.ptp(st.mesh.vertices, axis=0)

    def locate():
        elem, xi, ins = SpatiallyIndexed(st.mesh, eng, False).locate(pts)
        return np.concatenate([elem.astype(np.float64), xi.ravel(), ins.astype(np.float64)])

    route("points.locate", locate)
    if final:
        nodes = np.arange(0, st.mesh.num_nodes(), 7, dtype=np.uint64)
        eng.set_operator_dirichlet_nodes(nodes)
        matrix_free("dirichlet")
        eng.set_operator_dirichlet_nodes(st.dirichlet)
        matrix_free("dirichlet_taken_back")
        if st.density is None:
            eng.set_mass_density(RHO)   # (there is no call that takes a density back: the last route of an observation)
            shifted("density")
    return out, names


def _same(a, b):
    if isinstance(a, tuple) or isinstance(b, tuple):
        return a == b
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def compare_bitwise(got, fresh):
    """every array and every kernel name of the reused engine against the fresh one"""
    (ga, gn), (fa_, fn) = got, fresh
    assert ga.keys() == fa_.keys()
    bad = []
    for k in ga:
        is_array = not isinstance(ga[k], tuple) and not isinstance(fa_[k], tuple)
        if k in gn and is_array and k not in NO_KERNEL_OF_THEIR_OWN and gn[k] != fn[k]:
            bad.append(f"{k}: kernel '{gn[k]}' on the reused engine, '{fn[k]}' on the fresh one")
        if k in gn and is_array and gn[k] == fn[k] and any(part in HARDWARE_ORDER for part in gn[k].split(" + ")):
            continue
        if not _same(ga[k], fa_[k]):
            if isinstance(ga[k], tuple) or isinstance(fa_[k], tuple):
                bad.append(f"{k}: reused {ga[k] if isinstance(ga[k], tuple) else 'array'}, fresh {fa_[k] if isinstance(fa_[k], tuple) else 'array'}")
            else:
                bad.append(f"{k}: max |reused - fresh| = {np.abs(ga[k] - fa_[k]).max():.3e} (max |fresh| = {np.abs(fa_[k]).max():.3e})")
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------ the oracle on the final state
def _oracle_parts(oracle, st):
    """the oracle's assemblers whose sum is the final state: one per rule group, over the active elements"""
    conn = np.asarray(st.mesh.connectivity)
    active = np.ones(len(conn), dtype=bool) if st.mask is None else np.asarray(st.mask).astype(bool)
    groups = [(st.rule, active)] if st.rule is not None else [((w, p), active & (st.rules[1] == g)) for g, (w, p) in enumerate(st.rules[0])]
    parts = []
    for (w, p), sel in groups:
        kw = {}
        if st.op == "TENSOR":
            kw = {"tensor": st.tensor[0], "tensor_symmetric": st.tensor[1]}
        parts.append(oracle.ElementAssembler(st.mesh.elem_kind, getattr(oracle, st.op), st.mesh.vertices, conn[sel], w, p, params=np.asarray(LAME),
                                             u=st.u, **kw))
    return parts


def compare_oracle(oracle, st, got):
    arrays, _ = got
    s = st.sdim()
    full = oracle.ElementAssembler(st.mesh.elem_kind, getattr(oracle, st.op if st.op != "TENSOR" else "LINEAR_ELASTIC"), st.mesh.vertices,
                                   st.mesh.connectivity, *(st.rule or st.rules[0][0]), params=np.asarray(LAME))
    ro, ci = oracle.pattern_for(full)
    assert np.array_equal(arrays["pattern.row_offsets"], ro) and np.array_equal(arrays["pattern.col_indices"], ci), "pattern"
    parts = _oracle_parts(oracle, st)
    want = np.zeros(len(ci))
    want_r, want_e, want_f = np.zeros(s * st.mesh.num_nodes()), 0.0, np.zeros(s * st.mesh.num_nodes())
    linear_data = st.op == "TENSOR"   # an operator given as data has the matrix form only (FH_UNSUPPORTED for the residual and the energy)
    for part in parts:
        vals = np.zeros(len(ci))
        status, _ = oracle.assemble_into_csr(part, ro, ci, vals)
        assert status == 0
        want += vals
        if not linear_data:
            status, _, r = oracle.assemble_vector(part)
            assert status == 0
            want_r += r
            res = oracle.assemble_scalar(part)
            assert res[0] == 0
            want_e += res[-1]
        status, f = oracle.assemble_source_vector(part, s, g=GRAVITY[:s])
        assert status == 0
        want_f += f
    assert np.abs(want).max() > 0 and (linear_data or np.abs(want_r).max() > 0) and np.abs(want_f).max() > 0   # (the final state of a script is never trivial)
    lo, hi = (0, len(ci)) if st.rows is None else (int(ro[s * st.rows[0]]), int(ro[s * st.rows[1]]))
    in_range = np.zeros(len(ci), dtype=bool)
    in_range[lo:hi] = True
    bad = []
    scale = np.abs(want).max()
    for tag, _ in SCATTERS:
        for how, fill in (("accumulate", 0.0), ("overwrite", 7.0)):
            v = arrays[f"values.{tag}.{how}"]
            if isinstance(v, tuple):
                # a row range is served by the owner-computes kernels only (FH_UNSUPPORTED on the scatter kernels, documented)
                if not (st.rows is not None and tag != "gather" and v == ("error", 6)):   # (the reproducible form may need the two-pass kernels)
                    bad.append(f"values.{tag}.{how}: {v}")
                continue
            err = np.abs(v[in_range] - want[in_range]).max()
            print(f"values.{tag}.{how}: rel. err {err / scale:.2e}  [{got[1][f'values.{tag}.{how}']}]")
            if not err <= 1e-12 * scale:
                bad.append(f"values.{tag}.{how}: {err / scale:.3e} of max |want|")
            if not np.all(v[~in_range] == fill):
                bad.append(f"values.{tag}.{how}: rows outside the row range were written")
    for key, w in (("residual", want_r), ("energy", np.array([want_e])), ("source", want_f)):
        v = arrays[key]
        if isinstance(v, tuple):
            # the source assembler does not walk rule-set tables (FH_UNSUPPORTED, documented)
            if not (v == ("error", 6) and ((key == "source" and st.rules is not None) or (key != "source" and linear_data))):
                bad.append(f"{key}: {v}")
            continue
        err = np.abs(v - w).max()
        print(f"{key}: rel. err {err / np.abs(w).max():.2e}  [{got[1][key]}]")
        if not err <= 1e-12 * np.abs(w).max():
            bad.append(f"{key}: {err / np.abs(w).max():.3e} of max |want|")
    assert not bad, "\n".join(bad)


def drive(oracle, script):
    """the script on one long-lived engine, the final state alone on a fresh one; -> (state, reused observation, fresh observation)"""
    eng, st = fa.Engine(0), State()
    try:
        for step in script:
            if step is OBSERVE:
                observe(eng, st, final=False)
            else:
                step(eng, st)
        got = observe(eng, st)
    finally:
        eng.close()
    fresh_eng = fa.Engine(0)
    try:
        build(fresh_eng, st)
        fresh = observe(fresh_eng, st)
    finally:
        fresh_eng.close()
    compare_bitwise(got, fresh)
    compare_oracle(oracle, st, got)
    return st, got, fresh


# ------------------------------------------------------------------------------------------ the scripts
def test_meshes_of_other_sizes(oracle):
    """every buffer first too large, then too small: tiles, partition, affine records.  378 elements are two tiles, the second ragged"""
    script = (problem(_box(9, 7, 6), "LINEAR_ELASTIC", 1) + [OBSERVE] + problem(_box(5, 4, 3, 0.02, 2), "LINEAR_ELASTIC", 3) + [OBSERVE]
              + problem(_box(10, 8, 7), "LINEAR_ELASTIC", 4))
    drive(oracle, script)


@pytest.mark.parametrize("jitter", [0.0, 0.02])
def test_renumbering_with_the_same_sizes(oracle, jitter):
    """keys that compare sizes instead of generations: tiles, src_adj_gen, pattern, colours (same N, same E, other numbering)"""
    m = _box(9, 7, 6, jitter, 5)
    drive(oracle, problem(m, "LINEAR_ELASTIC", 6) + [OBSERVE] + problem(_permuted(m, 7), "LINEAR_ELASTIC", 8))


def _quad_then_tet(final_op, tensor_again=True):
    rng = np.random.default_rng(9)
    q = fa.procedural.create_unit_square_uniform_quad_mesh_2d(20)
    t = fa.procedural.create_unit_box_uniform_tet_mesh_3d(4)   # 768 elements
    wq, _ = _rule(fa.QUAD4)
    wt, _ = _rule(fa.TET4)
    assert len(wq) == len(wt) == 4   # the same nq, another d, another n
    script = problem(q, "LAPLACE", 10) + [OBSERVE, set_op("LINEAR_ELASTIC"), set_u(_u(q, "LINEAR_ELASTIC", 11)), OBSERVE,
                                         set_op("TENSOR"), set_tensor(rng.standard_normal((4, 2, 2, 2, 2))), OBSERVE]
    script += problem(t, final_op, 12)
    if final_op == "TENSOR" and tensor_again:
        script.append(set_tensor(rng.standard_normal((4, 3, 3, 3, 3))))
    return script


@pytest.mark.parametrize("final_op", ["LAPLACE", "LINEAR_ELASTIC", "TENSOR"])
def test_another_element_kind_under_the_same_point_count(oracle, final_op):
    """reference tables and tensor_nq: Quad4 with four points, then Tet4 with four points"""
    drive(oracle, _quad_then_tet(final_op))


def test_tensor_coefficients_go_with_the_mesh():
    """FH_TENSOR with 4 tensors of 2^4 doubles, then a Tet4 mesh and a four-point rule: nq matches, the buffer is 64 doubles where the kernels
    would read 4 x 81.  Every assembler answers FH_INVALID_STATE until fh_set_operator_tensor sends the coefficients again."""
    eng, st = fa.Engine(0), State()
    lib = eng._lib
    try:
        script = _quad_then_tet("TENSOR", tensor_again=False)
        for step in script:
            if step is not OBSERVE:
                step(eng, st)
        n = 3 * st.mesh.num_nodes()
        failed, nnz, energy = C.c_uint64(0), C.c_uint64(0), C.c_double(0.0)
        assert lib.fh_pattern(eng._h, None, C.byref(nnz)) == FH_OK
        values, vec, ke = np.zeros(int(nnz.value)), np.zeros(n), np.zeros(12 * 12)
        calls = {"fh_assemble_vector": lambda: lib.fh_assemble_vector(eng._h, _ffi.fp(vec), C.byref(failed)),
                 "fh_assemble_scalar": lambda: lib.fh_assemble_scalar(eng._h, C.byref(energy), C.byref(failed)),
                 "fh_assemble_element_matrices": lambda: lib.fh_assemble_element_matrices(eng._h, 0, 1, _ffi.fp(ke))}
        for flags in (fa.SCATTER_GATHER, fa.SCATTER_ATOMIC, fa.SCATTER_GATHER | fa.ASSEMBLE_OVERWRITE):
            calls[f"fh_assemble_matrix({flags:#x})"] = lambda f=flags: lib.fh_assemble_matrix(eng._h, _ffi.fp(values), f, C.byref(failed))
        for name, call in calls.items():
            assert call() == FH_INVALID_STATE, name
            assert "fh_set_operator_tensor" in eng.last_error(), name
        assert not values.any() and not vec.any() and not ke.any()
    finally:
        eng.close()


def test_hex27_between_hex8_meshes(oracle):
    """hex27_perm, gref_t_lex, tp_pos*, ke_dense: the two-pass tables of the quadratic kind across a linear one"""
    h27 = fa.hex27_mesh_from_hex8(fa.procedural.create_rectangular_uniform_hex_mesh(1.0, 2, 2, 3, 1))
    other = fa.hex27_mesh_from_hex8(fa.procedural.create_rectangular_uniform_hex_mesh(1.0, 3, 2, 2, 1))
    drive(oracle, problem(h27, "NEO_HOOKEAN", 13) + [OBSERVE] + problem(_box(4, 3, 3, 0.02, 14), "NEO_HOOKEAN", 15) + [OBSERVE]
          + problem(other, "NEO_HOOKEAN", 16))


@pytest.mark.parametrize("op", ["LAPLACE", "LINEAR_ELASTIC"])
@pytest.mark.parametrize("end", ["box again", "tolerance 0", "tolerance back"])
def test_vertex_updates_and_the_affine_tolerance(oracle, op, end):
    """classify_affine, a_recs_valid, a_shared and the quadrature-free residual (all_affine): an affine box, 2 % jitter, the box again, then
    the affine path switched off and on"""
    box = _box(6, 5, 4)
    moved = _box(6, 5, 4, 0.02, 17)
    script = problem(box, op, 18) + [OBSERVE, update_vertices(moved.vertices), OBSERVE, update_vertices(box.vertices)]
    if end != "box again":
        script += [OBSERVE, set_tol(0.0)]
    if end == "tolerance back":
        script += [OBSERVE, set_tol(2.0 ** -46)]
    drive(oracle, script)


@pytest.mark.parametrize("end", ["LINEAR_ELASTIC", "LAPLACE", "NEO_HOOKEAN"])
def test_operators_on_one_mesh(oracle, end):
    """the change of solution dim drops u; has_slotpar, the partition per operator, mf_scale_key"""
    m = _box(5, 4, 3, 0.02, 19)
    script = problem(m, "LINEAR_ELASTIC", 20) + [OBSERVE, set_op("LAPLACE")]
    if end != "LAPLACE":
        script += [set_u(_u(m, "LAPLACE", 21)), OBSERVE, set_op("NEO_HOOKEAN")]
        if end != "NEO_HOOKEAN":
            script += [set_u(_u(m, "NEO_HOOKEAN", 22)), OBSERVE, set_op("STABLE_NEO_HOOKEAN"), OBSERVE, set_op("LINEAR_ELASTIC")]
    st, _, _ = drive(oracle, script + ([set_u(_u(m, end, 23))] if end != "LINEAR_ELASTIC" else []))
    assert st.u is not None


def _mask(mesh, seed):
    return (np.random.default_rng(seed).random(mesh.num_elements()) < 0.6).astype(np.uint8)


@pytest.mark.parametrize("end", ["another mask", "no mask", "new mesh"])
def test_element_masks(oracle, end):
    """active_list, n2e_*_c, a_recs_gen, the coloured labels"""
    m = _box(6, 5, 4, 0.02, 24)
    script = problem(m, "LINEAR_ELASTIC", 25) + [OBSERVE, set_mask(_mask(m, 26)), OBSERVE]
    if end == "new mesh":
        script += problem(_box(5, 5, 3), "LINEAR_ELASTIC", 27)   # another E, no mask
    else:
        script += [set_mask(_mask(m, 28)), OBSERVE] + ([set_mask(None)] if end == "no mask" else [])
    drive(oracle, script)


@pytest.mark.parametrize("end", ["another range", "new mesh"])
def test_row_range(oracle, end):
    """row_lo / row_hi and the partition built for them"""
    m = _box(6, 5, 4, 0.02, 29)
    N = m.num_nodes()
    script = problem(m, "LINEAR_ELASTIC", 30) + [OBSERVE, set_rows(N // 3, 2 * N // 3), OBSERVE]
    script += [set_rows(N // 5, N // 2)] if end == "another range" else problem(_box(5, 4, 4), "LINEAR_ELASTIC", 31)
    drive(oracle, script)


def test_rows_stash_follows_a_vertex_update(oracle):
    """rows_stash.built_gen: the second set of tables of fh_assemble_matrix_rows_dev, then new vertices (other affine classes)"""
    import torch

    box, moved = _box(6, 5, 4), _box(6, 5, 4, 0.02, 32)
    N = box.num_nodes()
    lo, hi = N // 3, 2 * N // 3
    u = _u(box, "LINEAR_ELASTIC", 33)

    def rows(eng):
        ro, ci = eng.pattern()
        v = torch.full((len(ci),), 7.0, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        eng.assemble_matrix_rows(v, fa.SCATTER_GATHER | fa.ASSEMBLE_OVERWRITE, lo, hi)
        return ro, ci, v.cpu().numpy(), eng.last_kernel_name()

    eng, st = fa.Engine(0), State()
    try:
        for step in problem(box, "LINEAR_ELASTIC", 33):
            step(eng, st)
        rows(eng)
        eng.assemble_matrix(np.zeros(eng.nnz()), fa.SCATTER_GATHER)   # (the context's own tables, swapped with the stash around every rows call)
        update_vertices(moved.vertices)(eng, st)
        ro, ci, got, name = rows(eng)
    finally:
        eng.close()
    fresh = fa.Engine(0)
    try:
        build(fresh, st)
        _, _, want, want_name = rows(fresh)
    finally:
        fresh.close()
    assert got.tobytes() == want.tobytes() and name == want_name
    ref = oracle.ElementAssembler(oracle.HEX8, oracle.LINEAR_ELASTIC, moved.vertices, moved.connectivity, *_rule(fa.HEX8), params=np.asarray(LAME), u=u)
    status, _, oro, oci, vals = oracle.assemble(ref)
    assert status == 0 and np.array_equal(ro, oro) and np.array_equal(ci, oci)
    a, b = int(ro[3 * lo]), int(ro[3 * hi])
    assert np.abs(got[a:b] - vals[a:b]).max() <= 1e-12 * np.abs(vals).max()
    assert np.all(got[:a] == 7.0) and np.all(got[b:] == 7.0)


def _floor(stiffness=1.0e4):
    return [HalfSpace(point=(0.0, 0.0, 0.45), normal=(0.0, 0.0, 1.0), stiffness=stiffness)]   # the bottom layer of nodes (z = 0) penetrates


@pytest.mark.parametrize("end", ["none set", "set again"])
def test_dirichlet_nodes_density_and_obstacles_go_with_the_mesh(oracle, end):
    """mf_num_dirichlet, mass_rho_n, contact_clear: after a new mesh the matrix-free routes equal those of a fresh engine with none set (the
    shifted map without a density: FH_INVALID_STATE on both), and setting them again for the new mesh gives what a fresh engine gives"""
    a, b = _box(5, 4, 3, 0.02, 34), _box(4, 4, 4, 0.02, 35)
    script = problem(a, "NEO_HOOKEAN", 36) + [set_dirichlet(np.arange(0, a.num_nodes(), 3, dtype=np.uint64)), set_density(np.array([RHO])),
                                              set_obstacles(_floor()), OBSERVE] + problem(b, "NEO_HOOKEAN", 37)
    if end == "set again":
        script += [set_dirichlet(np.arange(1, b.num_nodes(), 4, dtype=np.uint64)), set_density(np.array([1.5 * RHO])), set_obstacles(_floor(2.0e4))]
    st, got, _ = drive(oracle, script)
    if end == "none set":
        assert got[0]["mf.shifted.state"] == ("error", FH_INVALID_STATE)   # no density: nothing of the old mesh's is applied
    else:
        assert not isinstance(got[0]["mf.shifted.state"], tuple)


def test_matrix_free_objects_hand_their_nodes_over_again_after_a_new_mesh():
    """the Python side of the same promise (Engine._mf_bound, _mass_bound, _contact_bound): an operator object that used the engine last
    before a new mesh must bind its nodes, density and obstacles again, and one without any must not inherit the old ones"""
    w, p = _rule(fa.HEX8)
    qt = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(fa.LameParameters(*LAME))
    a, b = _box(5, 4, 3, 0.02, 38), _box(4, 4, 4, 0.02, 39)
    x = np.cos(0.37 * np.arange(3 * b.num_nodes()))
    nodes = np.arange(1, b.num_nodes(), 4, dtype=np.uint64)

    def assembler(eng, m, seed):
        return (fa.ElementEllipticAssemblerBuilder(eng).with_finite_element_space(m).with_operator(fa.MaterialEllipticOperator(fa.NeoHookeanMaterial()))
                .with_quadrature_table(qt).with_u(_u(m, "NEO_HOOKEAN", seed)).build())

    def answers(eng, warm):
        if warm:
            old = assembler(eng, a, 40)
            op = fa.MatrixFreeShiftedTangent(old, RHO, 1.5, 0.25).with_dirichlet_nodes(np.arange(0, a.num_nodes(), 3, dtype=np.uint64)).with_obstacles(_floor())
            op.apply(np.zeros(3 * a.num_nodes()), np.cos(0.37 * np.arange(3 * a.num_nodes())))
        asm = assembler(eng, b, 41)
        plain = fa.MatrixFreeTangent(asm).apply(np.zeros_like(x), x)
        bound = fa.MatrixFreeShiftedTangent(asm, 1.5 * RHO, 1.5, 0.25).with_dirichlet_nodes(nodes).with_obstacles(_floor(2.0e4))
        first = bound.apply(np.zeros_like(x), x)
        eng.set_mesh(b)                       # the same mesh set again under the object: everything it owns is gone from the context
        assembler(eng, b, 41)
        again = bound.apply(np.zeros_like(x), x)
        return plain, first, again

    reused, fresh = fa.Engine(0), fa.Engine(0)
    try:
        got, want = answers(reused, True), answers(fresh, False)
    finally:
        reused.close()
        fresh.close()
    for g, w_ in zip(got, want):
        assert g.tobytes() == w_.tobytes()
    assert got[1].tobytes() == got[2].tobytes() and got[0].tobytes() != got[1].tobytes()


@pytest.mark.parametrize("end", ["rule set", "uniform"])
def test_rule_set_tables(oracle, end):
    """rs.active, rs.staged, user_mask: a table of two groups (2 and 3 points per direction), a new mesh with a uniform table, the rule set
    again -- and a user mask under the rule set, which the walk over the groups borrows"""
    a, b = _box(5, 4, 3, 0.02, 42), _box(4, 4, 3, 0.02, 43)
    groups = [quadrature.tensor.hexahedron_gauss(2), quadrature.tensor.hexahedron_gauss(3)]
    script = problem(a, "LINEAR_ELASTIC", 44) + [set_rules(groups, np.arange(a.num_elements()) % 2), set_mask(_mask(a, 45)), OBSERVE]
    script += problem(b, "LINEAR_ELASTIC", 46)
    if end == "rule set":
        script += [OBSERVE, set_rules(groups, (np.arange(b.num_elements()) // 3) % 2), set_mask(_mask(b, 47))]
    drive(oracle, script)


def test_ragged_connectivity_between_flat_meshes(oracle):
    """a flat mesh with a mask, a ragged connectivity of MORE elements, fh_pattern on it (the oracle's pattern), a flat mesh again: the ragged
    setter drops the mask, the rule-set flag, the table, u and moves topo_gen like the flat one (the module docstring has the finding)"""
    a, b = _box(4, 3, 3, 0.02, 48), _box(5, 4, 3, 0.02, 49)
    rng = np.random.default_rng(50)
    num_nodes = 150
    sizes = rng.integers(2, 7, size=3 * a.num_elements())
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    nodes = np.concatenate([rng.choice(num_nodes, size=k, replace=False) for k in sizes]).astype(np.uint64)

    def ragged(eng, st):
        eng.set_connectivity_ragged(2, num_nodes, offsets, nodes)
        ro, ci = eng.pattern()
        oro, oci = oracle.assemble_pattern(2, num_nodes, offsets, nodes)
        assert np.array_equal(ro, oro) and np.array_equal(ci, oci)
        failed = C.c_uint64(0)
        rc = eng._lib.fh_assemble_vector(eng._h, _ffi.fp(np.zeros(2 * num_nodes)), C.byref(failed))
        assert rc == FH_INVALID_STATE   # (no finite element mesh: nothing of the flat mesh is assembled)

    script = problem(a, "LINEAR_ELASTIC", 51) + [set_mask(_mask(a, 52)), OBSERVE, ragged] + problem(b, "LINEAR_ELASTIC", 53)
    drive(oracle, script)


def test_another_stream_between_two_assemblies(oracle):
    """a_recs_gen, and no hidden dependence on the old stream: the kept element records were enqueued on the stream the context had before"""
    import torch

    stream = torch.cuda.Stream()
    for m in (_box(6, 5, 4), _box(6, 5, 4, 0.02, 54)):
        drive(oracle, problem(m, "LINEAR_ELASTIC", 55) + [OBSERVE, set_stream(stream)])
    torch.cuda.synchronize()


def test_held_meshes_go_with_the_mesh():
    """held_drop_all after a plain fh_set_mesh: a held refinement, degree elevation and degree coarsening are gone, for the getters and for
    the contexts that would adopt them"""
    lin, quad, taker = fa.Engine(0), fa.Engine(0), fa.Engine(0)
    lib = lin._lib
    try:
        m8 = _box(3, 2, 2)
        m27 = fa.hex27_mesh_from_hex8(_box(2, 2, 2))
        lin.set_mesh(m8)
        quad.set_mesh(m27)
        nv_r, nc_r, _ = lin.refine_uniformly()
        nv_e, _ = lin.elevate_degree(fa.HEX27)
        nv_c, _ = quad.coarsen_degree()
        assert lin.refinement()[0].num_nodes() == nv_r and lin.degree_elevation()[0].num_nodes() == nv_e and quad.degree_coarsening()[0].num_nodes() == nv_c
        held = {"fh_refinement_mesh": (lin, np.zeros((nv_r, 3)), np.zeros((nc_r, 8), dtype=np.uint64), ()),
                "fh_degree_elevation_mesh": (lin, np.zeros((nv_e, 3)), np.zeros((m8.num_elements(), 27), dtype=np.uint64), ()),
                "fh_degree_coarsening_mesh": (quad, np.zeros((nv_c, 3)), np.zeros((m27.num_elements(), 8), dtype=np.uint64),
                                              (np.zeros(nv_c, dtype=np.uint64),))}
        lib.fh_set_mesh(lin._h, m8.elem_kind, _ffi.fp(m8.vertices), m8.num_nodes(), _ffi.up(m8.connectivity), m8.num_elements())
        lib.fh_set_mesh(quad._h, m27.elem_kind, _ffi.fp(m27.vertices), m27.num_nodes(), _ffi.up(m27.connectivity), m27.num_elements())
        for name, (eng, v, conn, extra) in held.items():
            assert getattr(lib, name)(eng._h, _ffi.fp(v), _ffi.up(conn), *[_ffi.up(x) for x in extra]) == FH_INVALID_STATE, name
            assert not v.any() and not conn.any()
        for name, eng in (("fh_set_mesh_from_refinement", lin), ("fh_set_mesh_from_degree_elevation", lin), ("fh_set_mesh_from_degree_coarsening", quad)):
            assert getattr(lib, name)(taker._h, eng._h) == FH_INVALID_STATE, name
        assert taker.num_nodes() == 0
    finally:
        for eng in (lin, quad, taker):
            eng.close()


# ------------------------------------------------------------------------------------------ handles made for a context
def _laplace_system(eng, k):
    """Quad4 k x k Laplace with the boundary clamped: (assembler, device CSR, rhs tensor, dense matrix)"""
    import torch

    m = fa.procedural.create_unit_square_uniform_quad_mesh_2d(k)
    w, p = _rule(fa.QUAD4)
    asm = (fa.ElementEllipticAssemblerBuilder(eng).with_finite_element_space(m).with_operator(fa.LaplaceOperator())
           .with_quadrature_table(fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(fa.LameParameters(*LAME)))
           .with_u(np.zeros(m.num_nodes())).build())
    csr = fa.CsrAssembler(fa.SCATTER_GATHER).assemble(asm, device_values=True)
    eng.apply_dirichlet_csr_dev(csr.values, eng.boundary_vertices())
    b = torch.from_numpy(np.sin(1.0 + np.arange(m.num_nodes()))).to("cuda:0")
    dense = fa.CsrMatrix(csr.row_offsets, csr.col_indices, csr.values.cpu().numpy()).to_scipy().toarray()
    return asm, csr, b, dense


def _converged(dense, b, x):
    """x solves the dense system: CG stopped at a relative residual of 1e-11 on its own recurrence, whose gap to the true residual is of
    the order eps cond(A) -- far below the 1e-10 asked of the true one here --, and ||x - x*|| <= cond(A) ||r|| / ||b|| ||x*||"""
    want = np.linalg.solve(dense, b)
    assert np.linalg.norm(b - dense @ x) <= 1e-10 * np.linalg.norm(b)
    assert np.linalg.norm(x - want) <= np.linalg.cond(dense) * 1e-10 * np.linalg.norm(want)


def _amg_solves(eng, csr, b, dense):
    import torch

    x = torch.zeros_like(b)
    eng.cg_solve(csr.values, b, x, fa.PRECOND_AMG, 1e-11)
    _converged(dense, b.cpu().numpy(), x.cpu().numpy())


@pytest.mark.parametrize("change", ["another mesh", "the same mesh again", "another solution dim"])
def test_amg_hierarchy_is_invalidated_with_its_pattern(change):
    """fh_amg_create keeps the context's noff / ncols pointers, N and nnz in level 0.  After fh_set_mesh + fh_pattern (another size, or the
    same mesh: equal sizes, new arrays) or an operator of another solution dim every entry that touches level 0 answers FH_INVALID_STATE
    with a message naming fh_amg_create, and a new hierarchy on the new state works.  A repeated fh_pattern on an UNCHANGED context builds
    nothing (build_pattern returns at has_pattern): the arrays stay and so does the hierarchy -- every Engine.pattern() call would otherwise
    end it."""
    import torch

    eng = fa.Engine(0)
    lib = eng._lib
    try:
        asm, csr, b, dense = _laplace_system(eng, 12)
        amg = fa.SmoothedAggregationAMG(asm, csr, near_nullspace="constant")
        _amg_solves(eng, csr, b, dense)
        eng.pattern()                       # fh_pattern again, nothing changed: still valid
        _amg_solves(eng, csr, b, dense)
        r, z, it = torch.ones_like(b), torch.zeros_like(b), C.c_uint64(0)
        if change == "another solution dim":
            eng.set_operator(_ffi.LINEAR_ELASTIC)
            r, z = torch.ones(2 * len(b), dtype=torch.float64, device="cuda:0"), torch.zeros(2 * len(b), dtype=torch.float64, device="cuda:0")
            values = torch.zeros(4 * len(csr.values), dtype=torch.float64, device="cuda:0")
            new = None
        else:
            new = _laplace_system(eng, 9 if change == "another mesh" else 12)   # fh_set_mesh, fh_pattern, an assembly
            values = new[1].values
            r, z = torch.ones_like(new[2]), torch.zeros_like(new[2])
        torch.cuda.synchronize()
        vp, rp, zp = (C.c_void_p(t.data_ptr()) for t in (values, r, z))
        stale = {"fh_cg_solve_dev": lambda: lib.fh_cg_solve_dev(eng._h, vp, rp, zp, fa.PRECOND_AMG, 1e-8, 0, C.byref(it)),
                 "fh_amg_apply_dev": lambda: lib.fh_amg_apply_dev(amg._h, rp, zp),
                 "fh_amg_update_values": lambda: lib.fh_amg_update_values(amg._h, vp),
                 "fh_amg_set_smoother": lambda: lib.fh_amg_set_smoother(amg._h, 2, 10.0, 8)}
        for name, call in stale.items():
            assert call() == FH_INVALID_STATE, name
            msg = eng.last_error()
            assert "fh_amg_create" in msg and "pattern changed" in msg and name.replace("_dev", "") in msg, (name, msg)
        assert not z.any().item() and it.value == 0
        amg.close()
        if new is not None:                 # a new hierarchy on the new state works
            amg2 = fa.SmoothedAggregationAMG(new[0], new[1], near_nullspace="constant")
            _amg_solves(eng, new[1], new[2], new[3])
            amg2.close()
        else:
            eng.set_operator(_ffi.LAPLACE)   # back to the solution dim of the values: a new hierarchy on them works
            amg2 = fa.SmoothedAggregationAMG(asm, csr, near_nullspace="constant")
            _amg_solves(eng, csr, b, dense)
            amg2.close()
    finally:
        eng.close()


@pytest.mark.parametrize("change", ["fine mesh of another size", "coarse mesh of another size", "another topology with the same size"])
def test_multigrid_hierarchy_is_invalidated_with_a_level_mesh(oracle, change):
    """fh_mg_create sizes the diagonal, the work vectors and the transfers per level.  After fh_set_mesh on the fine or the coarse context the
    multigrid solves and fh_mg_apply_dev answer FH_INVALID_STATE naming the level, before anything is written, and fh_mg_destroy returns"""
    import torch

    eng = fa.Engine(0)
    lib = eng._lib
    try:
        meshes, ts = fa.refine_uniformly_repeat_with_transfers(fa.procedural.create_unit_box_uniform_hex_mesh_3d(2), 1)   # 2^3 under 4^3
        fine = meshes[-1]
        w, p = _rule(fa.HEX8)
        qt = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(fa.LameParameters(*LAME))
        op = fa.MaterialEllipticOperator(fa.LinearElasticMaterial())

        def assembler(engine, m):
            return (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(m).with_operator(op).with_quadrature_table(qt)
                    .with_u(np.zeros(3 * m.num_nodes())).build())

        asm = assembler(eng, fine)
        mg = fa.GeometricMultigrid(asm, meshes[:-1], ts)
        clamp = np.where(np.isclose(fine.vertices[:, 0], 0.0))[0].astype(np.uint64)
        mf = fa.MatrixFreeOperator(asm).with_dirichlet_nodes(clamp).with_multigrid(mg)
        n = 3 * fine.num_nodes()
        b = np.sin(1.0 + np.arange(n))
        b.reshape(-1, 3)[clamp.astype(np.int64)] = 0.0
        x = np.zeros(n)
        mf.cg_solve(b, x, rel_tol=1e-11)
        # converged against a fresh solve: the oracle's matrix of the same problem, clamped the same way, solved densely
        ref = oracle.ElementAssembler(oracle.HEX8, oracle.LINEAR_ELASTIC, fine.vertices, fine.connectivity, w, p, params=np.asarray(LAME))
        status, _, ro, ci, vals = oracle.assemble(ref)
        assert status == 0
        oracle.apply_homogeneous_dirichlet_bc_csr(ro, ci, vals, clamp, 3)
        dense = fa.CsrMatrix(ro, ci, vals).to_scipy().toarray()
        _converged(dense, b, x)

        level, target = (0, mg.levels[0].engine) if change.startswith("coarse") else (1, eng)
        old = meshes[level]
        if change == "another topology with the same size":
            new = _permuted(old, 56)
        else:
            new = fa.procedural.create_unit_box_uniform_hex_mesh_3d(3 if level == 0 else 5)
        assembler(target, new)              # fh_set_mesh on that level's context, everything else set again
        if target is eng:
            eng.set_operator_dirichlet_nodes(np.zeros(0, dtype=np.uint64))
        n_new = 3 * eng.num_nodes()
        bt = torch.ones(n_new, dtype=torch.float64, device="cuda:0")
        xt = torch.zeros(n_new, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        it = C.c_uint64(0)
        bp, xp = C.c_void_p(bt.data_ptr()), C.c_void_p(xt.data_ptr())
        stale = {"fh_cg_solve_matrix_free": lambda: lib.fh_cg_solve_matrix_free_dev(eng._h, bp, xp, fa.PRECOND_MULTIGRID, 1e-8, 0, C.byref(it)),
                 "fh_cg_solve_tangent": lambda: lib.fh_cg_solve_tangent_dev(eng._h, bp, xp, fa.PRECOND_MULTIGRID, 1e-8, 0, C.byref(it)),
                 "fh_mg_apply_dev": lambda: lib.fh_mg_apply_dev(mg._h, 0.0, 1.0, bp, xp)}
        for name, call in stale.items():
            assert call() == FH_INVALID_STATE, name
            msg = eng.last_error()
            assert f"multigrid level {level}" in msg and "fh_mg_create" in msg, (name, msg)
        assert not xt.any().item() and it.value == 0
        mg._destroy()                       # fh_mg_destroy returns cleanly
        assert mg._h is None
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------ the comparison itself
def _unmodelled(step):
    """the step on the engine alone: the state the fresh engine is built from does not learn of it"""
    return lambda eng, st: step(eng, State())


@pytest.mark.parametrize("what", ["mask", "one vertex by 1e-9", "u", "Dirichlet nodes", "obstacles", "affine tolerance"])
def test_the_comparison_notices_state_one_engine_lacks(oracle, what):
    """the yardstick of this file: a setter that reaches only the long-lived engine -- what stale state in a cache amounts to -- must fail the
    comparison with the fresh engine"""
    m = _box(5, 4, 3)
    moved = m.vertices.copy()
    moved[7, 1] += 1e-9
    extra = {"mask": set_mask(_mask(m, 57)), "one vertex by 1e-9": lambda eng, st: eng.update_vertices(moved),
             "u": set_u(_u(m, "LINEAR_ELASTIC", 58)), "Dirichlet nodes": set_dirichlet(np.arange(0, m.num_nodes(), 5, dtype=np.uint64)),
             "obstacles": set_obstacles(_floor()), "affine tolerance": set_tol(0.0)}[what]
    with pytest.raises(AssertionError, match="reused"):
        drive(oracle, problem(m, "LINEAR_ELASTIC", 59) + [_unmodelled(extra)])
