"""The element records of the affine kernel (k_affine_records: R = sign(det J) rsqrt|det J| adj(J) per parallelepiped, M = R R^T for Laplace,
|det J| for the scalar mass) are kept across the assemblies of a context for as long as the vertices, the connectivity, the affine flags, the
mask and the record format stay (fenris_amd/csrc/engine_matrix.hip: launch_affine).  Every comparison here is bit for bit, against a FRESH
engine on the same inputs or against the same engine with FENRIS_HIP_AFFINE_RECORDS_ALWAYS=1; FENRIS_HIP_VERBOSE prints one line per records
pass that actually runs, which is how the tests see that the pass is skipped -- and that it comes back after everything that invalidates it."""
import numpy as np
import pytest

import fenris_amd as fa
from fenris_amd import distributed as fd
from fenris_amd import quadrature

pytestmark = pytest.mark.gpu
LAME = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.2))
LINE = "affine records computed"
OPS = {"LINEAR_ELASTIC": fa._ffi.LINEAR_ELASTIC, "LAPLACE": fa._ffi.LAPLACE, "MASS_SCALAR": fa._ffi.MASS_SCALAR}


def _box(n=10):
    return fa.procedural.create_unit_box_uniform_hex_mesh_3d(n)


def _sheared(mesh, A=((1.0, 0.3, 0.1), (0.0, 0.8, -0.2), (0.25, 0.0, 1.4)), b=(3.0, -1.0, 0.5)):
    """affine image of a mesh, as tests/test_affine.py builds it: every element stays a parallelepiped"""
    return fa.Mesh(mesh.vertices @ np.asarray(A, dtype=np.float64).T + np.asarray(b), mesh.connectivity, fa.HEX8)


def _mixed(n=10):
    """as tests/test_affine.py: the vertices of one corner region are perturbed, the rest stays affine"""
    rng = np.random.default_rng(5)
    m = _box(n)
    v = m.vertices.copy()
    sel = (v[:, 0] > 0.55) & (v[:, 1] > 0.35)
    v[sel] += 0.02 * rng.standard_normal((int(sel.sum()), 3))
    return fa.Mesh(v, m.connectivity, fa.HEX8)


def _perturbed(n=10):
    rng = np.random.default_rng(7)
    m = _box(n)
    return fa.Mesh(m.vertices + 0.1 / n * rng.uniform(-1, 1, m.vertices.shape), m.connectivity, fa.HEX8)


MESHES = {"box": lambda: _box(12), "sheared": lambda: _sheared(_box(10)), "mixed": _mixed}


def _set_operator(eng, op):
    """operator and quadrature table only: the mesh of the context stays as it is"""
    w, p = quadrature.tensor.hexahedron_gauss(2)
    qt = fa.UniformQuadratureTable.from_points_and_weights(p, w)
    if op == "LINEAR_ELASTIC":
        qt = qt.with_uniform_data(LAME)
    elif op == "MASS_SCALAR":
        qt = qt.with_data([fa.Density(1.0 + 0.125 * k) for k in range(len(w))])
    eng.set_operator(OPS[op])
    eng.set_quadrature_table(qt)
    eng.set_u(None)


def _setup(eng, mesh, op="LINEAR_ELASTIC"):
    eng.set_mesh(mesh)
    _set_operator(eng, op)


def _assemble(eng, overwrite=True, fill=-11.5, rows=None):
    import torch

    nnz = eng.build_pattern()
    v = torch.full((nnz,), fill if overwrite else 0.25, dtype=torch.float64, device="cuda:0")
    flags = fa.SCATTER_GATHER | (fa.ASSEMBLE_OVERWRITE if overwrite else 0)
    if rows is None:
        eng.assemble_matrix(v, flags)
    else:
        eng.assemble_matrix_rows(v, flags, rows[0], rows[1])
    return v


def _fresh(mesh, op="LINEAR_ELASTIC", overwrite=True, mask=None, tol=None):
    """what a new context makes of the same inputs"""
    eng = fa.Engine(0)
    try:
        _setup(eng, mesh, op)
        if tol is not None:
            eng.set_affine_tolerance(tol)
        if mask is not None:
            eng.set_active_elements(mask)
        return _assemble(eng, overwrite), eng.last_kernel_name()
    finally:
        eng.close()


def _fresh_range(mesh, rows, how):
    """a new context that has assembled nothing but the rows of the nodes [rows[0], rows[1]), into an array of -3.5"""
    eng = fa.Engine(0)
    try:
        _setup(eng, mesh)
        if how == "set_row_range":
            eng.set_row_range(*rows)
            return _assemble(eng, fill=-3.5)
        return _assemble(eng, fill=-3.5, rows=rows)
    finally:
        eng.close()


@pytest.fixture()
def engine():
    eng = fa.Engine(0)
    eng.set_option("FENRIS_HIP_VERBOSE", "1")
    yield eng
    eng.close()


def _lines(capfd):
    """records passes that ran since the last call"""
    return capfd.readouterr().err.count(LINE)


@pytest.mark.parametrize("overwrite", [True, False])
@pytest.mark.parametrize("op", ["LINEAR_ELASTIC", "LAPLACE", "MASS_SCALAR"])
@pytest.mark.parametrize("name", sorted(MESHES))
def test_three_assemblies_one_records_pass(engine, capfd, name, op, overwrite):
    import torch

    mesh = MESHES[name]()
    want, kern = _fresh(mesh, op, overwrite)
    if "k_affine_rows" not in kern:   # (the scalar mass of a mesh with a general block stays on the generic gather: nothing to keep)
        assert op == "MASS_SCALAR" and name == "mixed"
        return
    _setup(engine, mesh, op)
    _lines(capfd)
    for _ in range(3):
        assert torch.equal(_assemble(engine, overwrite), want)
        assert engine.last_kernel_name() == kern
    assert _lines(capfd) == 1
    # the switch brings the pass back into every assembly: same bits
    engine.set_option("FENRIS_HIP_AFFINE_RECORDS_ALWAYS", "1")
    for _ in range(3):
        assert torch.equal(_assemble(engine, overwrite), want)
    assert _lines(capfd) == 3
    engine.set_option("FENRIS_HIP_AFFINE_RECORDS_ALWAYS", None)
    assert torch.equal(_assemble(engine, overwrite), want)
    assert _lines(capfd) == 0


def test_update_vertices_refreshes_the_records(engine, capfd):
    import torch

    box = _box(10)
    _setup(engine, box)
    assert torch.equal(_assemble(engine), _fresh(box)[0])
    assert _lines(capfd) == 1
    # affine -> affine (another parallelepiped per element: same flags, the partition is kept), -> partly general, -> nothing affine, -> back
    for mesh, affine in ((_sheared(box), True), (_mixed(10), True), (_perturbed(10), False), (box, True)):
        engine.update_vertices(mesh.vertices)
        _lines(capfd)
        want, kern = _fresh(mesh)
        for _ in range(2):
            assert torch.equal(_assemble(engine), want)
            assert engine.last_kernel_name() == kern and ("k_affine_rows" in kern) == affine
        assert _lines(capfd) == (1 if affine else 0)


def test_set_mesh_refreshes_the_records(engine, capfd):
    import torch

    box = _box(10)
    _setup(engine, box)
    assert torch.equal(_assemble(engine), _fresh(box)[0])
    other = _sheared(box)     # same size: every buffer of the context is reused
    _setup(engine, other)
    _lines(capfd)
    want = _fresh(other)[0]
    assert torch.equal(_assemble(engine), want) and torch.equal(_assemble(engine), want)
    assert _lines(capfd) == 1


def test_affine_tolerance_refreshes_the_records(engine, capfd):
    import torch

    mesh = _mixed(10)
    _setup(engine, mesh)
    assert torch.equal(_assemble(engine), _fresh(mesh)[0])
    assert _lines(capfd) == 1
    for tol, affine in ((1e-7, True), (0.0, False), (2.0 ** -46, True)):
        engine.set_affine_tolerance(tol)
        want, kern = _fresh(mesh, tol=tol)
        assert ("k_affine_rows" in kern) == affine
        assert torch.equal(_assemble(engine), want) and torch.equal(_assemble(engine), want)
        assert engine.last_kernel_name() == kern
        assert _lines(capfd) == (1 if affine else 0)


@pytest.mark.parametrize("name", ["box", "mixed"])
def test_element_mask_on_and_off(engine, capfd, name):
    import torch

    mesh = MESHES[name]()
    _setup(engine, mesh)
    assert torch.equal(_assemble(engine), _fresh(mesh)[0])
    assert _lines(capfd) == 1
    active = (np.arange(mesh.num_elements()) % 5 != 2)
    for mask in (active, None, ~active, None):
        engine.set_active_elements(mask)
        want = _fresh(mesh, mask=mask)[0]
        assert torch.equal(_assemble(engine), want) and torch.equal(_assemble(engine), want)
        assert _lines(capfd) == 1


def test_operator_changes_refresh_the_records(engine, capfd):
    """one record set per context: elasticity (R), Laplace (R R^T) and the scalar mass (|det J|) each write their own format"""
    import torch

    mesh = _sheared(_box(10))
    engine.set_mesh(mesh)
    for op in ("LINEAR_ELASTIC", "LAPLACE", "MASS_SCALAR", "LAPLACE", "LINEAR_ELASTIC"):
        _set_operator(engine, op)
        _lines(capfd)
        want, kern = _fresh(mesh, op)
        assert kern == "k_affine_rows"
        assert torch.equal(_assemble(engine), want) and torch.equal(_assemble(engine), want)
        assert engine.last_kernel_name() == kern
        assert _lines(capfd) == 1


def test_placement_probe_in_the_middle(engine, capfd):
    """fh_tune_placement_dev exchanges the record buffer for candidate allocations: each candidate is filled by a records pass of its own,
    and whichever buffer the probe leaves behind, the next assembly reads current records"""
    import torch

    mesh = _box(12)
    _setup(engine, mesh)
    want = _fresh(mesh)[0]
    assert torch.equal(_assemble(engine), want)
    assert _lines(capfd) == 1
    vals = torch.zeros_like(want)
    flags = fa.SCATTER_GATHER | fa.ASSEMBLE_OVERWRITE
    tries = 3
    before, after = engine.tune_placement(vals, flags, tries=tries)
    assert 0.0 < after <= before and torch.equal(vals, want)
    assert _lines(capfd) >= tries              # one per candidate (the baseline timing before them reads the records it found)
    assert torch.equal(_assemble(engine), want)
    assert _lines(capfd) <= 1                  # 1: the last candidate was rejected and the old buffer came back; 0: it was kept
    assert torch.equal(_assemble(engine), want)
    assert _lines(capfd) == 0


@pytest.mark.parametrize("how", ["set_row_range", "assemble_matrix_rows"])
@pytest.mark.parametrize("name", sorted(MESHES))
def test_row_ranges_share_the_records(engine, capfd, name, how):
    """range A, the whole mesh, a disjoint range B, A again: what a fresh context makes of each range, which is the rows of the full assembly
    and nothing outside the range touched; once the whole mesh has been assembled the ranges find their records"""
    import torch

    mesh = MESHES[name]()
    full = _fresh(mesh)[0]
    _setup(engine, mesh)
    n = mesh.num_nodes()
    ro, _ = engine.pattern(want_cols=False)
    A, B = (n // 4, n // 2), (n // 2 + 7, n - 5)
    counts = []
    for rng_ in (A, None, B, A):
        _lines(capfd)
        if rng_ is None:
            if how == "set_row_range":
                engine.set_row_range(0, n)
            got = _assemble(engine)
            assert torch.equal(got, full)
        else:
            if how == "set_row_range":
                engine.set_row_range(*rng_)
                got = _assemble(engine, fill=-3.5)
            else:
                got = _assemble(engine, fill=-3.5, rows=rng_)
            lo, hi = int(ro[3 * rng_[0]]), int(ro[3 * rng_[1]])
            assert torch.equal(got, _fresh_range(mesh, rng_, how))
            if name != "mixed":   # (the general kernel's order of summation follows the blocks, which the range cuts anew: equal to rounding only)
                assert torch.equal(got[lo:hi], full[lo:hi])
            else:
                assert float((got[lo:hi] - full[lo:hi]).abs().max()) <= 1e-12 * float(full.abs().max())
            assert bool((got[:lo] == -3.5).all()) and bool((got[hi:] == -3.5).all())
        counts.append(_lines(capfd))
    assert counts[0] == 1 and counts[1] <= 1
    if name != "mixed":   # every element is affine: the whole mesh's records cover any range
        assert counts == [1, 1, 0, 0]


def _flat():
    # x' = x + z, y' = y, z' = 0 (tests/test_affine.py): every element is degenerate (det J == 0 exactly) and affine
    return _sheared(_box(4), [[1.0, 0.0, 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]], (0.0, 0.0, 0.0))


@pytest.mark.parametrize("op", ["LINEAR_ELASTIC", "LAPLACE"])
def test_singular_element_reported_by_every_assembly(engine, capfd, op):
    import torch

    flat = _flat()
    _setup(engine, flat, op)
    nnz = engine.build_pattern()
    vals = torch.zeros(nnz, dtype=torch.float64, device="cuda:0")
    flags = fa.SCATTER_GATHER | fa.ASSEMBLE_OVERWRITE
    for _ in range(3):
        with pytest.raises(fa.SingularJacobianError) as ei:
            engine.assemble_matrix(vals, flags)
        assert ei.value.element == 0
        assert engine.last_kernel_name() == "k_affine_rows"
    assert _lines(capfd) == 1     # the second and the third report come from the marks the pass left
    # the second status slot (fh_assemble_matrix_rows_dev): its own partition, the same records
    n = flat.num_nodes()
    for _ in range(3):
        with pytest.raises(fa.SingularJacobianError) as ei:
            engine.assemble_matrix_rows(vals, flags, 0, n)
        assert ei.value.element == 0
    # under a mask: the lowest ACTIVE failing element
    mask = np.ones(flat.num_elements(), dtype=np.uint8)
    mask[:5] = 0
    engine.set_active_elements(mask)
    for _ in range(3):
        with pytest.raises(fa.SingularJacobianError) as ei:
            engine.assemble_matrix(vals, flags)
        assert ei.value.element == 5


def test_masked_out_singular_element_stays_silent(engine, capfd):
    """a box with one detached, flattened (affine, det J == 0) element in front: masked out it is never reported, active it is reported by
    every assembly"""
    import torch

    box = _box(6)
    cube = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], dtype=np.float64)
    cube = cube @ np.array([[1.0, 0.0, 1.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]]).T   # the map of _flat: three non-zero edges in a plane
    nv = box.num_nodes()
    verts = np.concatenate([box.vertices, cube + np.array([5.0, 5.0, 5.0])])
    conn = np.concatenate([np.arange(nv, nv + 8, dtype=np.uint64)[None, :], np.asarray(box.connectivity, dtype=np.uint64)])
    mesh = fa.Mesh(verts, conn, fa.HEX8)
    mask = np.ones(mesh.num_elements(), dtype=np.uint8)
    mask[0] = 0
    _setup(engine, mesh)
    for m, raises in ((mask, False), (None, True), (mask, False)):
        engine.set_active_elements(m)
        _lines(capfd)
        if raises:
            nnz = engine.build_pattern()
            vals = torch.zeros(nnz, dtype=torch.float64, device="cuda:0")
            for _ in range(3):
                with pytest.raises(fa.SingularJacobianError) as ei:
                    engine.assemble_matrix(vals, fa.SCATTER_GATHER | fa.ASSEMBLE_OVERWRITE)
                assert ei.value.element == 0
        else:
            want = _fresh(mesh, mask=m)[0]
            for _ in range(3):
                assert torch.equal(_assemble(engine), want)
        assert engine.last_kernel_name().startswith("k_affine_rows")
        assert _lines(capfd) == 1


@pytest.mark.parametrize("rank", [0, 1])
def test_slab_step_settles_into_no_records_pass(capfd, rank):
    """both launches of a SlabAssembly step (the interface rows through the context's second set of tables, then the main range), for the two
    ranks of a two-slab cut on the one device: the second step equals the first bit for bit and runs no records pass"""
    import torch

    w, p = quadrature.tensor.hexahedron_gauss(2)
    qt = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(LAME)

    def configure(engine, mesh):
        return (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(mesh)
                .with_operator(fa.MaterialEllipticOperator(fa.LinearElasticMaterial())).with_quadrature_table(qt).with_u(None).build())

    slab = fd.make_slab(1.0, 1, 1, 2, 12, rank, 2)
    sa = fd.SlabAssembly(slab, configure, device=0, overlap=True, stream=torch.cuda.current_stream().cuda_stream)
    try:
        assert (sa.split is not None) == (rank == 1)
        sa.main.set_option("FENRIS_HIP_VERBOSE", "1")
        flags = fa.SCATTER_GATHER | fa.ASSEMBLE_OVERWRITE
        steps, lines = [], []
        for fill in (-11.5, 4.25, -0.5):
            _lines(capfd)
            sa.values.fill_(fill)
            if sa.split is not None:
                sa.main.assemble_matrix_rows_async(sa.values, flags, 0, sa.split)
            sa.main.assemble_matrix_async(sa.values, flags)
            sa.poll_status()
            torch.cuda.synchronize()
            assert "k_affine_rows" in sa.main.last_kernel_name()
            steps.append(sa.values.clone())
            lines.append(_lines(capfd))
        assert torch.equal(steps[1], steps[0]) and torch.equal(steps[2], steps[0])
        assert 1 <= lines[0] <= 2 and lines[1:] == [0, 0]
        # and the step is what the switch gives
        sa.main.set_option("FENRIS_HIP_AFFINE_RECORDS_ALWAYS", "1")
        sa.values.fill_(7.0)
        if sa.split is not None:
            sa.main.assemble_matrix_rows_async(sa.values, flags, 0, sa.split)
        sa.main.assemble_matrix_async(sa.values, flags)
        sa.poll_status()
        torch.cuda.synchronize()
        assert torch.equal(sa.values, steps[0])
        assert _lines(capfd) == (2 if sa.split is not None else 1)
    finally:
        sa.close()
