"""Matrix-free shifted tangent (alpha M + beta T(u)) x (fh_set_mass_density, fh_apply_shifted_tangent_dev, fh_shifted_tangent_diagonal_dev,
fh_cg_solve_shifted_tangent), the system of an implicit time step: against fh_spmv_dev on alpha M + beta K(u) assembled from the mass
assembler (the density as table data) and fh_assemble_matrix, |y - y_ref|_inf <= 1e-12 | (|alpha| |M| + |beta| |K|) |x| |_inf."""
import os

import numpy as np
import pytest

import fenris_amd as fa
from fenris_amd import _ffi, quadrature
from conftest import GOLDEN

LAME = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.3))
KINDS = ["QUAD4", "TRI3", "HEX8", "TET4", "QUAD9", "TRI6", "HEX20", "HEX27", "TET10", "TET20"]
NEW = ("fh_set_mass_density", "fh_apply_shifted_tangent_dev", "fh_shifted_tangent_diagonal_dev", "fh_cg_solve_shifted_tangent",
       "fh_cg_solve_shifted_tangent_dev")
FH_BAD_ARGUMENT, FH_INVALID_STATE, FH_UNSUPPORTED = 2, 5, 6


@pytest.fixture()
def engine():
    eng = fa.Engine(0)
    yield eng
    eng.close()


def _mesh(kind, res=3, seed=0, perturb=0.0):
    box3 = fa.procedural.create_unit_box_uniform_hex_mesh_3d
    tet3 = fa.procedural.create_unit_box_uniform_tet_mesh_3d
    quad2 = fa.procedural.create_unit_square_uniform_quad_mesh_2d
    tri2 = fa.procedural.create_unit_square_uniform_tri_mesh_2d
    make = {
        "QUAD4": (lambda: quad2(res), quadrature.tensor.quadrilateral_gauss(2)),
        "QUAD9": (lambda: fa.quad9_mesh_from_quad4(quad2(res)), quadrature.tensor.quadrilateral_gauss(3)),
        "TRI3": (lambda: tri2(res), quadrature.total_order.triangle(2)),
        "TRI6": (lambda: fa.tri6_mesh_from_tri3(tri2(res)), quadrature.total_order.triangle(4)),
        "HEX8": (lambda: box3(res), quadrature.tensor.hexahedron_gauss(2)),
        "HEX20": (lambda: fa.hex20_mesh_from_hex8(box3(2)), quadrature.tensor.hexahedron_gauss(3)),
        "HEX27": (lambda: fa.hex27_mesh_from_hex8(box3(2)), quadrature.tensor.hexahedron_gauss(3)),
        "TET4": (lambda: tet3(res), quadrature.total_order.tetrahedron(2)),
        "TET10": (lambda: fa.tet10_mesh_from_tet4(tet3(2)), quadrature.total_order.tetrahedron(4)),
        "TET20": (lambda: fa.tet20_mesh_from_tet4(tet3(1)), quadrature.total_order.tetrahedron(6)),
    }
    gen, (w, p) = make[kind]
    m = gen()
    if perturb:
        rng = np.random.default_rng(seed)
        m = fa.Mesh(m.vertices + perturb * rng.uniform(-1, 1, m.vertices.shape), m.connectivity, m.elem_kind)
    return m, np.asarray(w), np.asarray(p)


def _operator(op):
    return {"laplace": fa.LaplaceOperator(),
            "elastic": fa.MaterialEllipticOperator(fa.LinearElasticMaterial()),
            "neo_hookean": fa.MaterialEllipticOperator(fa.NeoHookeanMaterial()),
            "stvk": fa.MaterialEllipticOperator(fa.StVKMaterial())}[op]


def _sdim(m, op):
    return 1 if op == "laplace" else m.vertices.shape[1]


def _smooth_u(m, op, amp=0.05, seed=0):
    rng = np.random.default_rng(seed)
    x = m.vertices
    s = _sdim(m, op)
    u = np.zeros((len(x), s))
    for k in range(s):
        a = rng.uniform(-1, 1, 3)
        u[:, k] = amp * (a[0] * np.sin(np.pi * x[:, 0]) * np.cos(0.5 * np.pi * x[:, 1]) + a[1] * np.sin(np.pi * x[:, 1])
                         + a[2] * np.cos(np.pi * x.sum(axis=1)))
    return u.reshape(-1)


def _tables(op, table, w, p, m, second=None):
    """(stiffness table, rules [(w, p)], element -> rule) for the table forms; second: the rule-set's other rule (default Hex8 Gauss 3)"""
    nq, E = len(w), m.num_elements()
    zero = np.zeros(E, dtype=np.uint64)
    if table == "uniform":
        qt = fa.UniformQuadratureTable.from_points_and_weights(p, w)
        return (qt if op == "laplace" else qt.with_uniform_data(LAME)), [(w, p)], zero
    if table == "per_point":
        qt = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_data(
            [fa.LameParameters(1e5 * (1 + q), 2e5 * (2 + q % 3)) for q in range(nq)])
        return qt, [(w, p)], zero
    emap = (np.arange(E) % 3 == 0).astype(np.uint64)
    if table == "compact":
        rules = [(w, p, [fa.LameParameters(1e5 * (r + 1), 3e5 + q) for q in range(nq)]) for r in range(2)]
    else:   # rule_set: two point sets
        w2, p2 = (np.asarray(a) for a in (second or quadrature.tensor.hexahedron_gauss(3)))
        rules = [(w, p, [LAME] * nq), (w2, p2, [fa.LameParameters(2e5, 7e5)] * len(w2))]
    qt = fa.compact_quadrature_table([r[1] for r in rules], [r[0] for r in rules], [r[2] for r in rules], emap)
    return qt, [(r[0], r[1]) for r in rules], emap


def _mass_table(rules, emap, rho):
    """the density as table data for the assembled mass: one rule per element for a per-element density"""
    if np.ndim(rho) == 0:
        if len(rules) == 1:
            w, p = rules[0]
            return fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(fa.Density(float(rho)))
        return fa.compact_quadrature_table([r[1] for r in rules], [r[0] for r in rules],
                                           [[fa.Density(float(rho))] * len(r[0]) for r in rules], emap)
    E = len(emap)
    re = [rules[int(emap[e])] for e in range(E)]
    return fa.compact_quadrature_table([r[1] for r in re], [r[0] for r in re],
                                       [[fa.Density(float(rho[e]))] * len(re[e][0]) for e in range(E)], np.arange(E, dtype=np.uint64))


class _Ref:
    """alpha M + beta K(u) assembled on the same mesh (M on an engine of its own), with the Dirichlet modification"""

    def __init__(self, engine, m, op, qt, rules, emap, rho, u, alpha, beta, mask=None, bc=None):
        import torch

        s = _sdim(m, op)
        self.meng = fa.Engine(0)
        masm = fa.ElementMassAssembler.with_solution_dim(s, self.meng).with_space(m).with_quadrature_table(_mass_table(rules, emap, rho))
        if mask is not None:
            self.meng.set_active_elements(mask)
        km = fa.CsrAssembler(fa.SCATTER_GATHER).assemble(masm, device_values=True)
        self.asm = (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(m).with_operator(_operator(op))
                    .with_quadrature_table(qt).with_u(np.zeros(s * m.num_nodes()) if u is None else u).build())
        if mask is not None:
            engine.set_active_elements(mask)
        kk = fa.CsrAssembler(fa.SCATTER_GATHER).assemble(self.asm, device_values=True)
        assert np.array_equal(km.row_offsets, kk.row_offsets) and np.array_equal(km.col_indices, kk.col_indices)
        vals = torch.zeros_like(kk.values)
        if alpha != 0.0:
            vals += alpha * km.values
        if beta != 0.0:
            vals += beta * kk.values
        self.ms = fa.CsrMatrix(km.row_offsets, km.col_indices, km.values.cpu().numpy()).to_scipy()
        self.ks = fa.CsrMatrix(kk.row_offsets, kk.col_indices, kk.values.cpu().numpy()).to_scipy()
        self.full = fa.CsrMatrix(kk.row_offsets, kk.col_indices, vals.cpu().numpy()).to_scipy()   # before the Dirichlet rows
        self.a = fa.CsrMatrix(kk.row_offsets, kk.col_indices, vals)
        if bc is not None:
            fa.apply_homogeneous_dirichlet_bc_csr(self.a, bc, s, self.asm)
        self.engine, self.alpha, self.beta, self.s = engine, alpha, beta, s
        self.n = s * m.num_nodes()

    def close(self):
        self.meng.close()

    def apply(self, x):
        import torch

        y = torch.zeros(self.n, dtype=torch.float64, device="cuda")
        self.engine.spmv(self.a.values, x, y)
        return y.cpu().numpy()

    def bound(self, x):
        ax = np.abs(x.cpu().numpy())
        t = abs(self.alpha) * (abs(self.ms) @ ax)
        if self.beta != 0.0:
            t = t + abs(self.beta) * (abs(self.ks) @ ax)
        return np.abs(t).max()

    def scale(self):
        d = self.full.diagonal()
        nz = np.nonzero(d)[0]
        return abs(d[nz[0]]) if len(nz) else 1.0


def _check(ref, op, rng):
    import torch

    x = torch.from_numpy(rng.standard_normal(ref.n)).cuda()
    y = torch.full((ref.n,), float("nan"), dtype=torch.float64, device="cuda")   # overwritten: no NaN survives
    op.apply(y, x)
    y_ref = ref.apply(x)
    err = np.abs(y.cpu().numpy() - y_ref).max()
    bound = ref.bound(x)
    assert np.isfinite(err) and err <= 1e-12 * bound, (err, bound, ref.engine.last_kernel_name())
    return y


def test_shifted_entry_points_are_declared():
    """no GPU: the new entry points are in the header, the ctypes table and the Rust bindings"""
    root = os.path.join(os.path.dirname(GOLDEN), "..")
    hdr = open(os.path.join(root, "include", "fenris_hip.h")).read()
    rs = open(os.path.join(root, "bindings", "fenris_hip_sys.rs")).read()
    for name in NEW:
        assert name + "(" in hdr and name in _ffi.exported_symbols() and name in rs
    assert issubclass(fa.MatrixFreeShiftedTangent, fa.MatrixFreeOperator)
    assert issubclass(fa.MatrixFreeMass, fa.MatrixFreeShiftedTangent)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("op", ["laplace", "elastic"])   # s = 1 and s = d
@pytest.mark.parametrize("variant", ["uniform", "per_element_mask_dirichlet"])
def test_mass_matches_assembled_mass(engine, kind, op, variant):
    m, w, p = _mesh(kind, perturb=0.02, seed=1)
    rng = np.random.default_rng(3)
    E = m.num_elements()
    qt, rules, emap = _tables(op, "uniform", w, p, m)
    if variant == "uniform":
        rho, mask, bc = 2.5, None, None
    else:
        rho = rng.uniform(500.0, 1500.0, E)
        mask = rng.random(E) < 0.7
        bc = np.where(m.vertices[:, 0] < 1e-9)[0]
    ref = _Ref(engine, m, op, qt, rules, emap, rho, None, 1.0, 0.0, mask=mask, bc=bc)
    try:
        mass = fa.MatrixFreeMass(ref.asm, rho)
        if bc is not None:
            mass.with_dirichlet_nodes(bc)
        _check(ref, mass, rng)
        d_ref = ref.a.values.cpu().numpy()
        dm = fa.CsrMatrix(ref.a.row_offsets, ref.a.col_indices, d_ref).to_scipy().diagonal()
        assert np.abs(mass.diagonal() - dm).max() <= 1e-12 * np.abs(dm).max()
    finally:
        ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("perturb", [0.0, 0.03])   # all-affine box and general hexahedra
@pytest.mark.parametrize("table", ["per_point", "compact", "rule_set"])
def test_mass_hex8_tables(engine, perturb, table):
    m, w, p = _mesh("HEX8", res=4, perturb=perturb, seed=5)
    rng = np.random.default_rng(9)
    qt, rules, emap = _tables("elastic", table, w, p, m)
    rho = rng.uniform(1.0, 3.0, m.num_elements())
    ref = _Ref(engine, m, "stvk", qt, rules, emap, rho, _smooth_u(m, "stvk"), 1.5, 0.0)
    try:
        _check(ref, fa.MatrixFreeMass(ref.asm, rho).with_coefficients(1.5, 0.0), rng)
    finally:
        ref.close()


@pytest.mark.gpu
def test_mass_ignores_u_of_inverted_elements(engine):
    m, w, p = _mesh("HEX8", res=3)
    u = np.zeros(3 * m.num_nodes())
    u[3 * 13 + 0] = -5.0   # the centre node pushed through its elements: J < 0 there
    qt, rules, emap = _tables("neo_hookean", "uniform", w, p, m)
    ref = _Ref(engine, m, "neo_hookean", qt, rules, emap, 3.0, u, 2.0, 0.0)
    try:
        _check(ref, fa.MatrixFreeShiftedTangent(ref.asm, 3.0, 2.0, 0.0), np.random.default_rng(1))
    finally:
        ref.close()


SHIFT_CASES = [("HEX8", "uniform"), ("HEX8", "rule_set"), ("TET4", "uniform"), ("TET10", "uniform"), ("HEX27", "uniform"), ("QUAD4", "uniform")]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,table", SHIFT_CASES)
@pytest.mark.parametrize("op", ["neo_hookean", "stvk"])
def test_shifted_matches_assembled(engine, kind, table, op):
    m, w, p = _mesh(kind, perturb=0.02, seed=2)
    rng = np.random.default_rng(5)
    qt, rules, emap = _tables(op, table, w, p, m)
    bc = np.where(m.vertices[:, 0] < 1e-9)[0]
    rho = rng.uniform(800.0, 1200.0, m.num_elements())
    alpha, beta = 1.0, 1e-4
    ref = _Ref(engine, m, op, qt, rules, emap, rho, _smooth_u(m, op, seed=4), alpha, beta, bc=bc)
    try:
        t = fa.MatrixFreeShiftedTangent(ref.asm, rho, alpha, beta).with_dirichlet_nodes(bc)
        _check(ref, t, rng)
        d = t.diagonal()
        d_ref = fa.CsrMatrix(ref.a.row_offsets, ref.a.col_indices, ref.a.values.cpu().numpy()).to_scipy().diagonal()
        assert np.abs(d - d_ref).max() <= 1e-12 * np.abs(d_ref).max()
        # the Dirichlet rows hold the scale of the assembled alpha M + beta K(u)
        sc = ref.scale()
        fixed = (ref.s * bc[:, None] + np.arange(ref.s)).ravel()
        assert np.allclose(d[fixed], sc, rtol=1e-13, atol=0.0) and np.allclose(d_ref[fixed], sc, rtol=1e-13, atol=0.0)
    finally:
        ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("perturb", [0.0, 0.02])   # all-affine box (moment form of the mass) and general hexahedra (point form)
@pytest.mark.parametrize("op", ["laplace", "elastic", "neo_hookean", "stvk"])
@pytest.mark.parametrize("coef", [(1.0, 1e-4), (2.0, 0.0)])
def test_shifted_hex8_fused_pass(engine, perturb, op, coef):
    """Hex8 on the tiles: the mass term inside the monomial element pass (k_shifted_pass_tiled, k_shifted_tangent_tiled) or alone
    (k_mass_hex8_tiled), per-element density, Dirichlet nodes and an element mask"""
    import torch

    m, w, p = _mesh("HEX8", res=4, perturb=perturb, seed=12)
    rng = np.random.default_rng(13)
    qt, rules, emap = _tables(op, "uniform", w, p, m)
    E = m.num_elements()
    rho = rng.uniform(800.0, 1200.0, E)
    mask = rng.random(E) < 0.8
    bc = np.where(m.vertices[:, 0] < 1e-9)[0]
    alpha, beta = coef
    ref = _Ref(engine, m, op, qt, rules, emap, rho, _smooth_u(m, op, seed=3), alpha, beta, mask=mask, bc=bc)
    try:
        t = fa.MatrixFreeShiftedTangent(ref.asm, rho, alpha, beta).with_dirichlet_nodes(bc)
        y = _check(ref, t, rng)
        t.apply(y, torch.ones_like(y))   # (_check ends with the reference's SpMV: apply once more for the kernel's name)
        want = "k_mass_hex8_tiled" if beta == 0.0 else "k_shifted_pass_tiled" if op in ("laplace", "elastic") else "k_shifted_tangent_tiled"
        assert engine.last_kernel_name() == want + " + k_operator_from_partials", engine.last_kernel_name()
        d_ref = fa.CsrMatrix(ref.a.row_offsets, ref.a.col_indices, ref.a.values.cpu().numpy()).to_scipy().diagonal()
        assert np.abs(t.diagonal() - d_ref).max() <= 1e-12 * np.abs(d_ref).max()
    finally:
        ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["TET4", "HEX8"])
@pytest.mark.parametrize("op", ["elastic", "neo_hookean"])
def test_tiled_mass_and_shift_node_pass(engine, kind, op):
    """the tiles without the fused Hex8 pass (Tet4; Hex8 with the monomial form switched off): the tangent's own kernels, then k_mass_tiled
    and the shift node pass -- the name stays the tangent's, and with beta = 0 it is the mass pass's own.  More
    than one tile and one node-pass block, the last of each partial; per-element density, Dirichlet nodes and an element mask"""
    import torch

    m, w, p = _mesh(kind, res=7 if kind == "HEX8" else 5, perturb=0.01, seed=21)
    assert m.num_elements() > 256 and m.num_nodes() > 256
    rng = np.random.default_rng(22)
    if kind == "HEX8":
        engine.set_option("FENRIS_HIP_NO_MONOMIAL", "1")
    qt, rules, emap = _tables(op, "uniform", w, p, m)
    E = m.num_elements()
    rho = rng.uniform(800.0, 1200.0, E)
    mask = rng.random(E) < 0.8
    bc = np.where(m.vertices[:, 0] < 1e-9)[0]
    tangent = "k_element_pass_tiled + k_operator_from_partials" if op == "elastic" else "k_tangent_tiled + k_operator_from_partials"
    for alpha, beta in ((1.0, 1e-4), (2.0, 0.0)):
        ref = _Ref(engine, m, op, qt, rules, emap, rho, _smooth_u(m, op, seed=3), alpha, beta, mask=mask, bc=bc)
        try:
            t = fa.MatrixFreeShiftedTangent(ref.asm, rho, alpha, beta).with_dirichlet_nodes(bc)
            y = _check(ref, t, rng)
            t.apply(y, torch.ones_like(y))       # (_check ends with the reference's SpMV: apply once more for the kernel's name)
            assert engine.last_kernel_name() == (tangent if beta != 0.0 else "k_mass_tiled + k_shift_from_partials"), engine.last_kernel_name()
            d_ref = fa.CsrMatrix(ref.a.row_offsets, ref.a.col_indices, ref.a.values.cpu().numpy()).to_scipy().diagonal()
            assert np.abs(t.diagonal() - d_ref).max() <= 1e-12 * np.abs(d_ref).max()
        finally:
            ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["HEX27", "TET10", "QUAD9"])
def test_shifted_rule_set_groups_off_the_tiles(engine, kind):
    """k_mass_elements under a rule-set walk (quadratic kinds: no tiles), per-element density"""
    m, w, p = _mesh(kind, perturb=0.02, seed=14)
    second = {"HEX27": quadrature.tensor.hexahedron_gauss(2), "TET10": quadrature.total_order.tetrahedron(2),
              "QUAD9": quadrature.tensor.quadrilateral_gauss(4)}[kind]
    op = "neo_hookean"
    qt, rules, emap = _tables(op, "rule_set", w, p, m, second=second)
    rng = np.random.default_rng(15)
    rho = rng.uniform(1.0, 2.0, m.num_elements())
    bc = np.where(m.vertices[:, 0] < 1e-9)[0]
    for alpha, beta in ((1.0, 0.0), (1.0, 1e-5)):
        ref = _Ref(engine, m, op, qt, rules, emap, rho, _smooth_u(m, op, seed=6), alpha, beta, bc=bc)
        try:
            _check(ref, fa.MatrixFreeShiftedTangent(ref.asm, rho, alpha, beta).with_dirichlet_nodes(bc), rng)
        finally:
            ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["HEX8", "TET10"])
def test_alpha_zero_with_beta_scales_the_tangent(engine, kind):
    """alpha == 0, beta != 1: beta K(u) with the scale of beta K(u), and no density needed"""
    m, w, p = _mesh(kind, perturb=0.02, seed=16)
    op = "stvk"
    qt, rules, emap = _tables(op, "uniform", w, p, m)
    bc = np.where(m.vertices[:, 0] < 1e-9)[0]
    ref = _Ref(engine, m, op, qt, rules, emap, 1.0, _smooth_u(m, op, seed=7), 0.0, -2.5, bc=bc)
    try:
        t = fa.MatrixFreeShiftedTangent(ref.asm, 1.0, 0.0, -2.5).with_dirichlet_nodes(bc)
        _check(ref, t, np.random.default_rng(17))
        fixed = (3 * bc[:, None] + np.arange(3)).ravel()
        assert np.allclose(t.diagonal()[fixed], ref.scale(), rtol=1e-13, atol=0.0)
    finally:
        ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["HEX8", "TET4", "TET10"])
def test_alpha_zero_is_the_tangent_and_runs_repeat_bitwise(engine, kind):
    import torch

    m, w, p = _mesh(kind, perturb=0.02, seed=3)
    qt, _, _ = _tables("neo_hookean", "uniform", w, p, m)
    asm = (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(m).with_operator(_operator("neo_hookean"))
           .with_quadrature_table(qt).with_u(_smooth_u(m, "neo_hookean")).build())
    bc = np.where(m.vertices[:, 0] < 1e-9)[0]
    n = 3 * m.num_nodes()
    x = torch.from_numpy(np.random.default_rng(2).standard_normal(n)).cuda()
    tan = fa.MatrixFreeTangent(asm).with_dirichlet_nodes(bc)
    sh = fa.MatrixFreeShiftedTangent(asm, 1000.0, 0.0, 1.0).with_dirichlet_nodes(bc)
    yt, ys = torch.empty_like(x), torch.empty_like(x)
    tan.apply(yt, x)
    sh.apply(ys, x)
    assert torch.equal(yt, ys)
    assert np.array_equal(tan.diagonal(), sh.diagonal())
    # two runs of every entry point give identical bits (shifted coefficients, alternating with the plain map)
    sh.with_coefficients(1.0, 1e-3)
    outs = []
    for _ in range(2):
        y = torch.empty_like(x)
        sh.apply(y, x)
        tan.apply(yt, x)
        d = sh.diagonal()
        xs = torch.zeros_like(x)
        sh.cg_solve(x, xs, 1, 1e-10)
        outs.append((y.cpu().numpy(), d, xs.cpu().numpy()))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["HEX8", "TET4", "HEX27"])
def test_backward_euler_step_pcg_matches_assembled(engine, kind):
    import torch

    m, w, p = _mesh(kind, res=5 if kind != "HEX27" else 3, perturb=0.01, seed=6)
    op = "neo_hookean"
    qt, rules, emap = _tables(op, "uniform", w, p, m)
    bc = np.where(m.vertices[:, 0] < 1e-9)[0]
    dt, rho = 1e-3, 1000.0
    ref = _Ref(engine, m, op, qt, rules, emap, rho, _smooth_u(m, op, amp=0.01, seed=11), 1.0, dt * dt, bc=bc)
    try:
        n = ref.n
        b = np.random.default_rng(4).standard_normal(n)
        fa.apply_homogeneous_dirichlet_bc_rhs(b, bc, 3)
        xa = torch.zeros(n, dtype=torch.float64, device="cuda")
        it_a = (fa.ConjugateGradient.new().with_operator(ref.a, ref.asm).with_preconditioner(fa.JacobiPreconditioner())
                .with_stopping_criterion(fa.RelativeResidualCriterion(1e-11)).solve_with_guess(torch.from_numpy(b).cuda(), xa))
        t = fa.MatrixFreeShiftedTangent(ref.asm, rho, 1.0, dt * dt).with_dirichlet_nodes(bc)
        xm = torch.zeros(n, dtype=torch.float64, device="cuda")
        it_m = (fa.ConjugateGradient.new().with_operator(t).with_preconditioner(fa.JacobiPreconditioner())
                .with_stopping_criterion(fa.RelativeResidualCriterion(1e-11)).solve_with_guess(torch.from_numpy(b).cuda(), xm))
        assert abs(it_a - it_m) <= 1, (it_a, it_m)
        xa, xm = xa.cpu().numpy(), xm.cpu().numpy()
        assert np.abs(xa - xm).max() <= 1e-9 * np.abs(xa).max()
        xh = np.zeros(n)   # host form: the same iterate
        t.cg_solve(b, xh, 1, 1e-11)
        assert np.array_equal(xh, xm)
    finally:
        ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["HEX8", "TET10", "QUAD9"])
def test_lumped_mass_is_the_row_sum(engine, kind):
    m, w, p = _mesh(kind, perturb=0.02, seed=8)
    op = "elastic"
    qt, rules, emap = _tables(op, "uniform", w, p, m)
    ref = _Ref(engine, m, op, qt, rules, emap, 7.0, None, 1.0, 0.0)
    try:
        mass = fa.MatrixFreeMass(ref.asm, 7.0).with_dirichlet_nodes([0, 1])   # (lumped() ignores the Dirichlet nodes)
        lm = mass.lumped()
        rs = np.asarray(ref.ms.sum(axis=1)).ravel()
        assert np.abs(lm - rs).max() <= 1e-12 * np.abs(rs).max()
    finally:
        ref.close()
    if kind == "HEX8":   # a box: sum = s rho V
        box, w, p = _mesh("HEX8", res=4)
        asm = (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(box).with_operator(_operator(op))
               .with_quadrature_table(fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(LAME))
               .with_u(np.zeros(3 * box.num_nodes())).build())
        vol = np.prod(box.vertices.max(axis=0) - box.vertices.min(axis=0))
        assert abs(fa.MatrixFreeMass(asm, 7.0).lumped().sum() - 3 * 7.0 * vol) <= 1e-12 * 3 * 7.0 * vol


@pytest.mark.gpu
def test_shifted_contract(engine):
    import torch

    m, w, p = _mesh("HEX8", res=3)
    qt, rules, emap = _tables("stvk", "uniform", w, p, m)
    asm = (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(m).with_operator(_operator("stvk"))
           .with_quadrature_table(qt).with_u(_smooth_u(m, "stvk")).build())
    lib, h = engine._lib, engine._h
    n = 3 * m.num_nodes()
    x = torch.ones(n, dtype=torch.float64, device="cuda")
    y = torch.empty_like(x)
    xp, yp = x.data_ptr(), y.data_ptr()
    # no density: FH_INVALID_STATE for alpha != 0; alpha == 0 needs none
    assert lib.fh_apply_shifted_tangent_dev(h, 1.0, 1.0, xp, yp) == FH_INVALID_STATE
    assert lib.fh_apply_shifted_tangent_dev(h, 0.0, 2.0, xp, yp) == 0
    # bad counts
    rho = np.full(m.num_elements() + 1, 2.0)
    assert lib.fh_set_mass_density(h, _ffi.fp(rho), 2) == FH_BAD_ARGUMENT
    assert lib.fh_set_mass_density(h, _ffi.fp(rho), m.num_elements() + 1) == FH_BAD_ARGUMENT
    assert lib.fh_set_mass_density(h, None, 1) == FH_BAD_ARGUMENT
    assert lib.fh_set_mass_density(h, _ffi.fp(rho), m.num_elements()) == 0
    assert lib.fh_apply_shifted_tangent_dev(h, 1.0, 1.0, xp, yp) == 0
    # the density changes the Dirichlet scale (the cache key holds the density's counter)
    bc = np.where(m.vertices[:, 0] < 1e-9)[0]
    engine.set_operator_dirichlet_nodes(bc)
    d = torch.empty_like(x)
    assert lib.fh_shifted_tangent_diagonal_dev(h, 1.0, 1e-6, d.data_ptr()) == 0
    assert lib.fh_apply_shifted_tangent_dev(h, 1.0, 1e-6, xp, yp) == 0
    row = 3 * int(bc[0])
    s1 = y[row].item()
    assert s1 == d[row].item()
    assert lib.fh_set_mass_density(h, _ffi.fp(4.0 * rho), 1) == 0
    assert lib.fh_apply_shifted_tangent_dev(h, 1.0, 1e-6, xp, yp) == 0
    s2 = y[row].item()
    assert s2 != s1
    # plain and shifted calls alternate: each gets its own scale back
    assert lib.fh_apply_tangent_dev(h, xp, yp) == 0
    st = y[row].item()
    assert lib.fh_apply_shifted_tangent_dev(h, 1.0, 1e-6, xp, yp) == 0
    assert y[row].item() == s2 and st != s2
    # fh_set_mesh drops the density
    asm2 = (fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(m).with_operator(_operator("stvk"))
            .with_quadrature_table(qt).with_u(_smooth_u(m, "stvk")).build())
    assert asm2.engine is engine
    assert lib.fh_apply_shifted_tangent_dev(h, 1.0, 1.0, xp, yp) == FH_INVALID_STATE
    # mass and tensor operators: FH_UNSUPPORTED
    mq = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(fa.Density(1.0))
    fa.ElementMassAssembler.with_solution_dim(3, engine).with_space(m).with_quadrature_table(mq)
    assert lib.fh_set_mass_density(h, _ffi.fp(rho), 1) == 0
    assert lib.fh_apply_shifted_tangent_dev(h, 1.0, 1.0, xp, yp) == FH_UNSUPPORTED
    assert lib.fh_shifted_tangent_diagonal_dev(h, 1.0, 0.0, d.data_ptr()) == FH_UNSUPPORTED
