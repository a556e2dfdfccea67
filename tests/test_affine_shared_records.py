"""Shared form of the affine sweep's loader (fenris_amd/csrc/affine_rows.hip, engine_matrix.hip: affine_shared_prepare): affine elements whose
records agree bit for bit share one entry of a table of distinct records, node blocks whose slots hold the same classes share one slot list,
and the sweep reads the two small tables instead of one record per element and one list per block.  "Identical" below is torch.equal on the
whole values array between the shared loader and FENRIS_HIP_AFFINE_SHARED=0 in the SAME context; every case is also held against the oracle
at the tolerance of tests/test_affine.py.  The engines of these tests build the tables in the first assembly of a mesh generation
(FENRIS_HIP_AFFINE_SHARED_AFTER=0); test_build_waits_for_an_unchanged_mesh holds the default, which defers the build."""
import numpy as np
import pytest

import fenris_amd as fa
from fenris_amd import quadrature

pytestmark = pytest.mark.gpu
TOL = 1e-12
LAME = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.2))
OPS = {"LINEAR_ELASTIC": fa._ffi.LINEAR_ELASTIC, "LAPLACE": fa._ffi.LAPLACE}
FLAGS = fa.SCATTER_GATHER | fa.ASSEMBLE_OVERWRITE


def _box_15x4x3():
    """15 x 4 x 3 cells of unit / 15: several distinct edge lengths per axis (i / 15 rounds differently along a line), 16 nodes = three
    node blocks per line"""
    return fa.procedural.create_rectangular_uniform_hex_mesh(1.0 / 15.0, 15, 4, 3, 1)


def _graded(nx=9, ny=4, nz=3, shear=True, power=1.7):
    """tensor-product grading with a global shear: every element is a parallelepiped, no two neighbours along an axis are congruent"""
    g = fa.procedural.create_rectangular_uniform_hex_mesh(1.0, nx, ny, nz, 1)
    v = g.vertices / np.array([nx, ny, nz], dtype=np.float64)
    v = np.stack([v[:, 0] ** power, 2.0 * v[:, 1] ** 0.8, np.expm1(v[:, 2])], axis=1)
    if shear:
        v = v @ np.array([[1.0, 0.3, 0.1], [0.0, 0.8, -0.2], [0.25, 0.0, 1.4]]).T + np.array([3.0, -1.0, 0.5])
    return fa.Mesh(v, g.connectivity, fa.HEX8)


def _mixed():
    """the graded box with a few perturbed (non-affine) elements and a hole (two elements removed)"""
    m = _graded(9, 5, 4, shear=False)
    rng = np.random.default_rng(11)
    v = m.vertices.copy()
    idx = rng.choice(len(v), 4, replace=False)
    v[idx] += 0.004 * rng.standard_normal((4, 3))
    conn = np.asarray(m.connectivity)
    keep = np.ones(len(conn), dtype=bool)
    keep[[67, 68]] = False
    return fa.Mesh(v, conn[keep], fa.HEX8)


def _setup(eng, mesh, op):
    w, p = quadrature.tensor.hexahedron_gauss(2)
    qt = fa.UniformQuadratureTable.from_points_and_weights(p, w)
    if op == "LINEAR_ELASTIC":
        qt = qt.with_uniform_data(LAME)
    eng.set_mesh(mesh)
    eng.set_operator(OPS[op])
    eng.set_quadrature_table(qt)
    eng.set_u(None)


def _assemble(eng):
    import torch

    v = torch.full((eng.build_pattern(),), -11.5, dtype=torch.float64, device="cuda:0")
    eng.assemble_matrix(v, FLAGS)
    return v


def _both(eng, expect_shared=True, op="LINEAR_ELASTIC"):
    """(values of the shared loader, its stats, values of the per-element loader in the same context); Laplace has the shared loader only
    where FENRIS_HIP_AFFINE_SHARED=1 asks for it (it is slower there)"""
    on = "1" if op == "LAPLACE" else None
    eng.set_option("FENRIS_HIP_AFFINE_SHARED", on)
    shared = _assemble(eng)
    st = eng.affine_shared_stats()
    assert st["shared"] == expect_shared, st
    eng.set_option("FENRIS_HIP_AFFINE_SHARED", "0")
    plain = _assemble(eng)
    off = eng.affine_shared_stats()
    assert not off["shared"] and "FENRIS_HIP_AFFINE_SHARED" in off["reason"]
    eng.set_option("FENRIS_HIP_AFFINE_SHARED", on)
    return shared, st, plain


def _oracle_values(oracle, mesh, op):
    w, p = quadrature.tensor.hexahedron_gauss(2)
    if op == "LAPLACE":
        ref = oracle.ElementAssembler(oracle.HEX8, oracle.LAPLACE, mesh.vertices, mesh.connectivity, w, p, params=None)
    else:
        ref = oracle.ElementAssembler(oracle.HEX8, oracle.LINEAR_ELASTIC, mesh.vertices, mesh.connectivity, w, p, params=LAME.as_pair())
    st, _, _, _, vals = oracle.assemble(ref)
    assert st == 0
    return vals


def _close(values, vals):
    return np.abs(values.cpu().numpy() - vals).max() <= TOL * np.abs(vals).max()


def _restated_counts(mesh, slot_elements):
    """what the tables must hold, from the vertices: a record is a function of the bits of the three edge vectors from node 0 to nodes 1, 3, 4
    (k_affine_records), a list is the classes of a block's slots with 0xffff for an empty one"""
    v = np.asarray(mesh.vertices, dtype=np.float64)
    c = np.asarray(mesh.connectivity).astype(np.int64)
    edges = np.concatenate([v[c[:, k]] - v[c[:, 0]] for k in (1, 3, 4)], axis=1)
    _, cls = np.unique(np.ascontiguousarray(edges).view(np.uint64), axis=0, return_inverse=True)
    cls = cls.reshape(-1)
    lists = np.where(slot_elements < 0, 0xffff, cls[np.maximum(slot_elements, 0)])
    return int(cls.max()) + 1, len(np.unique(lists, axis=0))


@pytest.fixture()
def engine():
    eng = fa.Engine(0)
    eng.set_option("FENRIS_HIP_AFFINE_SHARED_AFTER", "0")
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def box_reference(oracle):
    mesh = _box_15x4x3()
    return mesh, {op: _oracle_values(oracle, mesh, op) for op in OPS}


@pytest.mark.parametrize("grid", [None, "2"])
@pytest.mark.parametrize("op", sorted(OPS))
def test_structured_box_non_dyadic_spacing(engine, box_reference, op, grid):
    """grid = 2: one workgroup walks many blocks and crosses changes of slot list and of lane table in both parities of the double buffer"""
    import torch

    mesh, refs = box_reference
    if grid:
        engine.set_option("FENRIS_HIP_AFFINE_GRID", grid)
    _setup(engine, mesh, op)
    shared, st, plain = _both(engine, op=op)
    assert engine.last_kernel_name() == "k_affine_rows"
    assert torch.equal(shared, plain)
    assert _close(shared, refs[op])
    nrec, nvec = _restated_counts(mesh, engine.affine_slot_elements())
    print(f"records {st['records']} (restated {nrec}) of {mesh.num_elements()} elements, lists {st['lists']} (restated {nvec})")
    assert nrec > 3 and st["records"] == nrec and st["lists"] == nvec


@pytest.mark.parametrize("op", sorted(OPS))
def test_graded_and_sheared_box(engine, oracle, op):
    import scipy.sparse as sp
    import torch

    mesh = _graded()
    _setup(engine, mesh, op)
    shared, st, plain = _both(engine, op=op)
    assert engine.last_kernel_name() == "k_affine_rows" and st["records"] > 1
    assert torch.equal(shared, plain)
    assert torch.equal(_assemble(engine), shared) and engine.affine_shared_stats()["shared"]   # reproducible over two runs
    assert _close(shared, _oracle_values(oracle, mesh, op))
    ro, ci = engine.pattern()
    n = len(ro) - 1
    A = sp.csr_matrix((shared.cpu().numpy(), ci.astype(np.int64), ro.astype(np.int64)), shape=(n, n))
    D = (A - A.T).tocoo()
    assert D.nnz == 0 or not np.any(D.data != 0.0)


def test_over_the_limits(engine, oracle):
    import torch

    mesh = _graded()
    _setup(engine, mesh, "LINEAR_ELASTIC")
    first = _assemble(engine)
    st = engine.affine_shared_stats()
    assert st["shared"] and st["records"] > 2 and st["lists"] > 2
    for name, word in (("FENRIS_HIP_AFFINE_SHARED_MAX_RECORDS", "records"), ("FENRIS_HIP_AFFINE_SHARED_MAX_LISTS", "lists")):
        engine.set_option(name, "2")
        got = _assemble(engine)
        off = engine.affine_shared_stats()
        assert not off["shared"] and word in off["reason"] and "limit" in off["reason"], off
        assert torch.equal(got, first)
        assert torch.equal(_assemble(engine), first) and not engine.affine_shared_stats()["shared"]
        engine.set_option(name, None)
        assert torch.equal(_assemble(engine), first) and engine.affine_shared_stats() == st
    assert _close(first, _oracle_values(oracle, mesh, "LINEAR_ELASTIC"))


def _fresh(mesh, op="LINEAR_ELASTIC", tol=None):
    eng = fa.Engine(0)
    eng.set_option("FENRIS_HIP_AFFINE_SHARED_AFTER", "0")
    try:
        _setup(eng, mesh, op)
        if tol is not None:
            eng.set_affine_tolerance(tol)
        return _assemble(eng), eng.affine_shared_stats(), eng.last_kernel_name()
    finally:
        eng.close()


def test_mesh_changes(engine, oracle):
    import torch

    a, b = _graded(power=1.7), _graded(power=1.3)
    _setup(engine, a, "LINEAR_ELASTIC")
    _assemble(engine)
    engine.update_vertices(b.vertices)
    want, st, _ = _fresh(b)
    shared, st2, plain = _both(engine)
    assert torch.equal(shared, want) and torch.equal(plain, want) and st2 == st
    assert _close(shared, _oracle_values(oracle, b, "LINEAR_ELASTIC"))
    # the tolerance decides which elements qualify: the slightly perturbed ones of the mixed mesh join the class at 1e-7
    m = _mixed_slight()
    _setup(engine, m, "LINEAR_ELASTIC")
    before = _assemble(engine)
    n_before = engine.affine_stats()[0]
    engine.set_affine_tolerance(1e-7)
    want, st, kern = _fresh(m, tol=1e-7)
    shared, st2, plain = _both(engine, expect_shared=st["shared"])
    assert engine.affine_stats()[0] > n_before and engine.last_kernel_name() == kern
    assert torch.equal(shared, want) and torch.equal(plain, want) and st2 == st
    # (at the loosened tolerance the affine form differs from the oracle by O(tolerance): the fresh context above is the reference there)
    assert _close(before, _oracle_values(oracle, m, "LINEAR_ELASTIC"))


def _mixed_slight():
    """graded box, four vertices moved by 1e-10 of the box: general at the default tolerance, affine at 1e-7"""
    m = _graded(9, 5, 4, shear=False)
    v = m.vertices.copy()
    idx = np.random.default_rng(3).choice(len(v), 4, replace=False)
    v[idx] += 1e-10
    return fa.Mesh(v, m.connectivity, fa.HEX8)


@pytest.mark.parametrize("op", sorted(OPS))
def test_mixed_mesh(engine, oracle, op):
    import torch

    mesh = _mixed()
    _setup(engine, mesh, op)
    shared, st, plain = _both(engine, op=op)
    n_aff, n_aff_blk, n_gen_blk = engine.affine_stats()
    assert engine.last_kernel_name().startswith("k_affine_rows + ") and n_aff_blk > 0 and n_gen_blk > 0 and 0 < n_aff < mesh.num_elements()
    assert torch.equal(shared, plain)
    assert _close(shared, _oracle_values(oracle, mesh, op))


def test_laplace_default_keeps_the_loader(engine):
    """the Laplace sweep is not bound by memory and the shared loader is slower there: off unless asked for"""
    mesh = _graded()
    _setup(engine, mesh, "LAPLACE")
    _assemble(engine)
    st = engine.affine_shared_stats()
    assert not st["shared"] and "FENRIS_HIP_AFFINE_SHARED=1" in st["reason"] and engine.last_kernel_name() == "k_affine_rows"


def test_singular_element(engine):
    """one affine element with det J == 0: status and element index as the per-element loader reports them, on the assembly that runs the
    records pass and on the next one, which replays the marks"""
    import torch

    g = _graded(6, 4, 3, shear=False)
    v = g.vertices.copy()
    conn = np.asarray(g.connectivity)
    nv = len(v)
    cube = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], dtype=np.float64)
    flat = cube @ np.array([[1.0, 0.0, 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]]).T + 5.0   # three non-zero edges in a plane, detached
    at = 7
    mesh = fa.Mesh(np.concatenate([v, flat]), np.concatenate([conn[:at], np.arange(nv, nv + 8, dtype=conn.dtype)[None, :], conn[at:]]), fa.HEX8)
    _setup(engine, mesh, "LINEAR_ELASTIC")
    vals = torch.zeros(engine.build_pattern(), dtype=torch.float64, device="cuda:0")
    got = {}
    for mode in ("shared", "plain"):
        engine.set_option("FENRIS_HIP_AFFINE_SHARED", None if mode == "shared" else "0")
        engine.update_vertices(mesh.vertices)   # the next assembly runs the records pass, the one after replays
        for k in range(2):
            with pytest.raises(fa.SingularJacobianError) as ei:
                engine.assemble_matrix(vals, FLAGS)
            assert engine.affine_shared_stats()["shared"] == (mode == "shared")
            got[mode, k] = (ei.value.element, vals.clone())
    for k in range(2):
        assert got["shared", k][0] == got["plain", k][0] == at
        assert torch.equal(got["shared", k][1], got["plain", k][1])


def test_masked_context_keeps_the_loader(engine):
    import torch

    mesh = _graded()
    _setup(engine, mesh, "LINEAR_ELASTIC")
    active = (np.arange(mesh.num_elements()) % 5 != 2)
    engine.set_active_elements(active)
    masked = _assemble(engine)
    st = engine.affine_shared_stats()
    assert not st["shared"] and "mask" in st["reason"] and engine.last_kernel_name().startswith("k_affine_rows")
    engine.set_option("FENRIS_HIP_AFFINE_SHARED", "0")
    assert torch.equal(_assemble(engine), masked)
    engine.set_option("FENRIS_HIP_AFFINE_SHARED", None)
    ka = torch.zeros_like(masked)
    engine.assemble_matrix(ka, fa.SCATTER_ATOMIC | fa.ASSEMBLE_OVERWRITE)
    assert float((masked - ka).abs().max()) <= TOL * float(ka.abs().max())
    engine.set_active_elements(None)
    _assemble(engine)
    assert engine.affine_shared_stats()["shared"]


def test_build_waits_for_an_unchanged_mesh(oracle):
    """the default: the build costs tens of assemblies, so the first two sweeps of a mesh generation keep the per-element loader, twice as
    many after every build in a row that ended over a limit; fh_time_assembly_dev builds in its untimed first assembly.  Same bits throughout."""
    import torch

    mesh = _graded()
    eng = fa.Engine(0)
    try:
        _setup(eng, mesh, "LINEAR_ELASTIC")
        first = _assemble(eng)
        assert _close(first, _oracle_values(oracle, mesh, "LINEAR_ELASTIC"))

        def sweeps(n):
            out = []
            for _ in range(n):
                assert torch.equal(_assemble(eng), first)
                st = eng.affine_shared_stats()
                out.append("shared" if st["shared"] else "waiting" if "not built yet" in st["reason"] else st["reason"])
            return out

        assert not eng.affine_shared_stats()["shared"] and "not built yet" in eng.affine_shared_stats()["reason"]
        assert sweeps(3) == ["waiting", "shared", "shared"]
        eng.update_vertices(mesh.vertices)          # a new generation of the same vertices
        assert sweeps(3) == ["waiting", "waiting", "shared"]
        eng.update_vertices(mesh.vertices)
        vals = torch.zeros_like(first)
        eng.time_assembly(vals, FLAGS, 1)           # its set-up assembly builds at once
        assert torch.equal(vals, first) and eng.affine_shared_stats()["shared"]
        # over a limit: the next generations wait twice, then four times as long
        eng.set_option("FENRIS_HIP_AFFINE_SHARED_AFTER", "1")
        eng.set_option("FENRIS_HIP_AFFINE_SHARED_MAX_RECORDS", "2")
        got = sweeps(2)
        assert got[0] == "waiting" and "limit" in got[1]
        eng.update_vertices(mesh.vertices)
        got = sweeps(3)
        assert got[:2] == ["waiting", "waiting"] and "limit" in got[2]
        eng.update_vertices(mesh.vertices)
        got = sweeps(5)
        assert got[:4] == ["waiting"] * 4 and "limit" in got[4]
        eng.set_option("FENRIS_HIP_AFFINE_SHARED_MAX_RECORDS", None)   # a build that fits ends the doubling
        assert sweeps(9) == ["waiting"] * 8 + ["shared"]
        eng.update_vertices(mesh.vertices)
        assert sweeps(2) == ["waiting", "shared"]
    finally:
        eng.close()


def test_placement_swaps_the_record_buffer(engine, oracle):
    """FENRIS_HIP_PLACEMENT_KEEP=1: the probe keeps every candidate, so the record buffer behind the assemblies that follow IS another one;
    the tables hold copies of record values and stay"""
    import torch

    mesh = _graded()
    _setup(engine, mesh, "LINEAR_ELASTIC")
    before = _assemble(engine)
    st = engine.affine_shared_stats()
    assert st["shared"]
    vals = torch.zeros_like(before)
    engine.set_option("FENRIS_HIP_PLACEMENT_KEEP", "1")
    engine.tune_placement(vals, FLAGS, tries=2)
    engine.set_option("FENRIS_HIP_PLACEMENT_KEEP", None)
    assert torch.equal(vals, before)
    after = _assemble(engine)
    assert torch.equal(after, before) and engine.affine_shared_stats() == st
    assert _close(after, _oracle_values(oracle, mesh, "LINEAR_ELASTIC"))
