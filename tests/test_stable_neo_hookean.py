"""FH_STABLE_NEO_HOOKEAN against the long-double reference of tests/stable_neo_hookean_reference.py: the law that stays finite through
inversion.

Meshes, cases (a) .. (e), routes and bars are those of test_large_deformation.py (imported, not restated).  Three more deformations:
  (f) F = diag(1, 1, -0.3) (2-D: diag(1, -0.3)) with the shear of case (a): every element reflected, det F < 0 at every point,
  (g) F of rank d - 1: the box pressed flat into the plane x_d = 0, det F = 0 at every point,
  (h) case (d) with one node of one element in twenty pushed through the opposite side of that element: both signs of det F (asserted).
For (f), (g), (h) every output of every route is finite and no element is reported as failed.
Bars (none loosened): K 1e-12 max|K|, apply 1e-12 || |K| |x| ||, diagonal 1e-12 max|d|, residual 1e-12 of its absolute scale, energy 1e-12
sum |psi_e|, under the rigid rotation the magnitudes of the terms of P and psi; recovery at points 1e-12 of the largest term magnitude."""
import numpy as np
import pytest

import fenris_amd as fa
import hp_reference as hp
import stable_neo_hookean_reference as snh
import test_large_deformation as tld
from test_large_deformation import BAR, F2, F3, R2, R3, RHO, mesh_of

LD = np.longdouble
F3_NEW = {"f": np.array([[1.0, 0.4, 0.0], [0.0, 1.0, 0.3], [0.2, 0.0, -0.3]]),
          "g": np.array([[1.0, 0.4, 0.0], [0.0, 1.0, 0.3], [0.0, 0.0, 0.0]])}
F2_NEW = {"f": np.array([[1.0, 0.4], [0.2, -0.3]]), "g": np.array([[1.0, 0.4], [0.0, 0.0]])}
INVERTED = ("f", "g", "h")


def params_of(case, d):
    """the law's own (mu, lambda) whose linearisation is the Lame pair of the case"""
    return tld.lame_of(case).for_stable_neo_hookean(d)


def deformation(case, X, conn=None):
    d = X.shape[1]
    if case in ("f", "g"):
        F = (F3_NEW if d == 3 else F2_NEW)[case]
        return (X @ (F - np.eye(d)).T).reshape(-1)
    if case != "h":
        return tld.deformation(case, X)
    x = X + tld.deformation("d", X).reshape(-1, d)
    lo, hi = X.min(axis=0), X.max(axis=0)
    interior = np.all((X > lo + 1e-9) & (X < hi - 1e-9), axis=1)
    moved = set()
    for e in range(0, len(conn), 20):
        nodes = [int(n) for n in conn[e]]
        pick = next((n for n in nodes if interior[n] and n not in moved), None)
        if pick is None:
            continue
        moved.add(pick)
        c = np.mean([x[n] for n in nodes if n != pick], axis=0)
        x[pick] += 2.2 * (c - x[pick])          # through the centroid of the element's other nodes and out on the far side
    assert len(moved) >= 3
    return (x - X).reshape(-1)


def reference(kind, m, w, p, u, case, **kw):
    lm = params_of(case, m.vertices.shape[1])
    ref = snh.Reference(kind, m.vertices, m.connectivity, w, p, u, lm.mu, lm.lambda_, rho=RHO, **kw)
    if case == "f":
        assert ref.det_F_max < 0.0
    elif case == "g":
        assert max(abs(ref.det_F_min), abs(ref.det_F_max)) <= 1e-14
    elif case == "h":
        assert ref.det_F_min < 0.0 < ref.det_F_max
    else:
        assert ref.det_F_min > 0.0
    return ref


# ------------------------------------------------------------------------------------------------------------------ CPU: the reference itself
def _rand_F(d, n, seed, inverted):
    rng = np.random.default_rng(seed)
    F = np.eye(d) + 0.6 * rng.standard_normal((n, d, d))
    F[hp.det(F) < 0, 0] *= -1        # (a row's sign is the determinant's)
    if inverted:
        F[:, 0] *= -1
    return F.astype(LD)


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("inverted", [False, True])
def test_stress_is_the_derivative_of_the_energy(d, inverted):
    """P = d psi / d F by central differences in long double, at det F > 0 and at det F < 0"""
    F = _rand_F(d, 12, d, inverted)
    assert np.all((hp.det(F) < 0) == inverted)
    mu, lam, I = LD(3.0), LD(5.0), np.eye(d, dtype=LD)
    P = snh.stress(F, mu, lam, I)[0]
    h = LD(1e-8)
    for i in range(d):
        for j in range(d):
            dF = np.zeros((d, d), dtype=LD)
            dF[i, j] = h
            fd = (snh.stress(F + dF, mu, lam, I)[1] - snh.stress(F - dF, mu, lam, I)[1]) / (2 * h)
            assert np.abs(fd - P[:, i, j]).max() <= 1e-10 * np.abs(P).max()


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("inverted", [False, True])
def test_contraction_is_the_derivative_of_the_stress(d, inverted):
    """C(a, b)[i][k] = sum_jl a_j (dP_ij / dF_kl) b_l by central differences of P, and C(b, a) = C(a, b)^T"""
    F = _rand_F(d, 6, 10 + d, inverted)
    mu, lam, I = LD(3.0), LD(5.0), np.eye(d, dtype=LD)
    g = np.random.default_rng(5).standard_normal((6, 2, d)).astype(LD)     # two "nodes": a = g[:, 0], b = g[:, 1]
    C = snh.contraction(F, g, mu, lam, I)
    h = LD(1e-8)
    dP = np.zeros((6, d, d, d, d), dtype=LD)
    for k in range(d):
        for l in range(d):
            dF = np.zeros((d, d), dtype=LD)
            dF[k, l] = h
            dP[:, :, :, k, l] = (snh.stress(F + dF, mu, lam, I)[0] - snh.stress(F - dF, mu, lam, I)[0]) / (2 * h)
    fd = np.einsum("ej,eijkl,el->eik", g[:, 0], dP, g[:, 1])
    assert np.abs(fd - C[:, 0, :, 1, :]).max() <= 1e-9 * np.abs(C).max()
    assert np.abs(C[:, 1, :, 0, :] - np.swapaxes(C[:, 0, :, 1, :], 1, 2)).max() <= 1e-17 * np.abs(C).max()


@pytest.mark.parametrize("kind", tld.KINDS)
@pytest.mark.parametrize("case", ["a", "f"])
def test_reference_derivatives_by_central_differences(kind, case):
    """K x = (r(u + h x) - r(u - h x)) / 2h and r . x = (E(u + h x) - E(u - h x)) / 2h on a mesh, at det F > 0 and det F < 0"""
    m, (w, p) = tld._small(kind, seed=2)
    w, p = np.asarray(w), np.asarray(p)
    u = deformation(case, m.vertices)
    lm = params_of(case, m.vertices.shape[1])
    x = np.random.default_rng(3).standard_normal(u.size).astype(LD)
    h = LD(1e-7)

    def at(v):
        return snh.Reference(kind, m.vertices, m.connectivity, w, p, v, lm.mu, lm.lambda_)

    ref, rp, rm = at(u), at(u.astype(LD) + h * x), at(u.astype(LD) - h * x)
    assert (ref.det_F_max < 0) if case == "f" else (ref.det_F_min > 0)
    kx = ref.apply(x)[0]
    fd = (rp.residual() - rm.residual()) / (2 * h)
    assert np.abs(fd - kx).max() <= 1e-9 * np.abs(kx).max(), float(np.abs(fd - kx).max() / np.abs(kx).max())
    rx = np.dot(ref.residual(), x)
    fe = (rp.energy() - rm.energy()) / (2 * h)
    assert abs(fe - rx) <= 1e-9 * np.dot(ref.residual_scale(), np.abs(x))


@pytest.mark.parametrize("d", [2, 3])
def test_rest_state_and_frame_indifference(d):
    I = np.eye(d, dtype=LD)
    mu, lam = LD(3.0), LD(5.0)
    P, psi, _, _ = snh.stress(I[None], mu, lam, I)
    assert not np.any(P) and psi[0] == 0
    R = (R3 if d == 3 else R2).astype(LD)
    for inverted in (False, True):
        F = _rand_F(d, 8, 20 + d, inverted)
        P, psi, _, _ = snh.stress(F, mu, lam, I)
        Pr, psir, _, _ = snh.stress(R[None] @ F, mu, lam, I)          # exact rotations: R F is a signed permutation of the rows of F
        assert np.abs(psir - psi).max() <= 4e-19 * np.abs(psi).max()
        assert np.abs(Pr - R[None] @ P).max() <= 4e-19 * np.abs(P).max()
    P, psi, _, _ = snh.stress(R[None], mu, lam, I)                    # a rigid rotation: no stress, no energy
    assert np.abs(P).max() <= 1e-18 * float(mu) and abs(psi[0]) <= 1e-18 * float(mu)


@pytest.mark.parametrize("kind", tld.KINDS)
def test_linearisation_at_rest_is_linear_elasticity(kind):
    m, (w, p) = tld._small(kind, seed=1)
    w, p = np.asarray(w), np.asarray(p)
    d = m.vertices.shape[1]
    lm = tld.LAME.for_stable_neo_hookean(d)
    u0 = np.zeros(m.vertices.size)
    k = snh.Reference(kind, m.vertices, m.connectivity, w, p, u0, lm.mu, lm.lambda_).ke
    kl = hp.Reference(kind, "LINEAR_ELASTIC", m.vertices, m.connectivity, w, p, u0, tld.LAME.mu, tld.LAME.lambda_).ke
    assert np.abs(k - kl).max() <= 1e-15 * np.abs(kl).max(), float(np.abs(k - kl).max() / np.abs(kl).max())


@pytest.mark.parametrize("kind", ["HEX8", "TET4", "QUAD4", "TRI3"])
@pytest.mark.parametrize("case", ["f", "g"])
def test_everything_finite_when_inverted_or_flat(kind, case):
    m, (w, p) = tld._small(kind)
    w, p = np.asarray(w), np.asarray(p)
    ref = reference(kind, m, w, p, deformation(case, m.vertices), case)
    for a in (ref.ke, ref.re, ref.psi, ref.re_scale, ref.psi_term):
        assert np.all(np.isfinite(a.astype(np.float64)))


def test_parameter_conversion_against_the_closed_form():
    import ctypes as C
    from fenris_amd import _ffi

    for d in (2, 3):
        for mu_l, lam_l in ((1.0, 0.0), (3.846153846153846e5, 5.769230769230769e5), (0.3, 70.0)):
            got = fa.LameParameters(mu_l, lam_l).for_stable_neo_hookean(d)
            mu, lam = snh.parameters(d, mu_l, lam_l)
            assert abs(got.mu - mu) <= 2e-16 * mu and abs(got.lambda_ - lam) <= 4e-16 * (abs(lam_l) + mu_l)
            # ... which linearise back: mu_L = mu d/(d+1), lambda_L = lambda + 2 mu/(d+1)^2 - mu d/(d+1)
            assert abs(mu * d / (d + 1) - mu_l) <= 4e-16 * mu_l
            assert abs(lam + 2 * mu / (d + 1) ** 2 - mu * d / (d + 1) - lam_l) <= 1e-15 * (abs(lam_l) + mu_l)
    out = C.c_double()
    assert _ffi.lib().fh_stable_neo_hookean_parameters(4, 1.0, 1.0, C.byref(out), C.byref(out)) == _ffi.FH_BAD_ARGUMENT
    assert _ffi.lib().fh_stable_neo_hookean_parameters(1, 1.0, 1.0, C.byref(out), C.byref(out)) == _ffi.FH_BAD_ARGUMENT
    assert _ffi.lib().fh_stable_neo_hookean_parameters(3, 1.0, 1.0, None, C.byref(out)) == _ffi.FH_BAD_ARGUMENT
    with pytest.raises(fa.FenrisError):
        fa.LameParameters(1.0, 1.0).for_stable_neo_hookean(1)
    assert fa.StableNeoHookeanMaterial.op_kind == fa.STABLE_NEO_HOOKEAN == 7


def test_case_h_mixes_the_signs_of_det_F():
    kind, m, w, p = mesh_of("TET4")
    reference(kind, m, w, p, deformation("h", m.vertices, m.connectivity), "h")


# ------------------------------------------------------------------------------------------------------------------ GPU: every route
OP = "STABLE_NEO_HOOKEAN"
GPU_CASES = [(v, c) for v in tld.VARIANTS
             for c in ("a", "b", "e", "f", "g") + (("c", "d", "h") if v in ("HEX8_AFFINE", "HEX8_GENERAL", "TET4") else ())]
_assert_le = tld._assert_le     # records error / bar under its key and asserts; the keys of this module carry OP


@pytest.fixture(scope="module", autouse=True)
def _print_margins():
    yield
    mine = {k: v for k, v in tld.MARGINS.items() if OP in k}
    if mine:
        print("\nlargest error / bar per route and deformation:")
        for k in sorted(mine):
            print(f"  {k:80s} {mine[k]:.3f}")


def _table(w, p, lame):
    return fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(lame)


def _builder(engine, m, qt, u, material=None):
    op = fa.MaterialEllipticOperator((material or fa.StableNeoHookeanMaterial)())
    return fa.ElementEllipticAssemblerBuilder(engine).with_finite_element_space(m).with_operator(op).with_quadrature_table(qt).with_u(u).build()


def _host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _mask_and_reproducible(engine, asm, kind, ref, tag):
    """an element mask (every third element off) and FH_ASSEMBLE_REPRODUCIBLE twice for equal bits"""
    out = {}
    k1 = fa.CsrAssembler(fa.SCATTER_GATHER | fa.ASSEMBLE_REPRODUCIBLE).assemble(asm)
    v1 = tld._check_k(f"K {kind} reproducible {tag}", k1, ref)
    v2 = _host(fa.CsrAssembler(fa.SCATTER_GATHER | fa.ASSEMBLE_REPRODUCIBLE).assemble(asm).values)
    assert np.array_equal(v1.view(np.uint64), v2.view(np.uint64))
    out["reproducible"] = v1
    mask = (np.arange(len(ref.ke)) % 3 != 1).astype(np.uint8)
    engine.set_active_elements(mask)
    try:
        k = fa.CsrAssembler(fa.SCATTER_GATHER).assemble(asm)
        kh = ref._on_pattern(ref.ke * mask[:, None, None].astype(ref.dt))
        out["mask"] = _host(k.values)
        _assert_le(f"K {kind} element mask {tag}", np.abs(out["mask"] - kh).max(), np.abs(kh).max())
    finally:
        engine.set_active_elements(None)
    return out


def _recovery(engine, kind, m, p, u, lame, case, tag):
    """the five quantities at the points.  Cauchy and von Mises are P F^T / det F: compared where det F > 0, NaN where every point is inverted"""
    ref = snh.at_points(kind, m.vertices, m.connectivity, p, u, lame.mu, lame.lambda_)
    d = m.vertices.shape[1]
    F, P = ref["F"], ref["P"]
    aF = np.abs(F)
    got = {q: _host(engine.recover(q, "points")) for q in ("grad_u", "strain", "stress_pk1", "cauchy_stress", "von_mises", "energy_density")}
    _assert_le(f"recover grad_u {tag}", np.abs(got["grad_u"] - ref["grad_u"]).max(), np.abs(ref["grad_u"]).max())
    I = np.eye(d, dtype=LD)
    E = (np.einsum("eki,ekj->eij", F, F) - I) / 2
    _assert_le(f"recover strain {tag}", np.abs(got["strain"] - E).max(), ((np.einsum("eki,ekj->eij", aF, aF) + I) / 2).max())
    _assert_le(f"recover stress_pk1 {tag}", np.abs(got["stress_pk1"] - P).max(), ref["P_abs"].max())
    _assert_le(f"recover energy_density {tag}", np.abs(got["energy_density"] - ref["psi"]).max(), ref["psi_abs"].max())
    out = [got[q] for q in ("grad_u", "strain", "stress_pk1", "energy_density")]
    J = hp.det(F)
    if case == "f":
        assert np.isnan(got["cauchy_stress"]).all() and np.isnan(got["von_mises"]).all()
    elif case not in INVERTED:
        sig = np.einsum("eik,ejk->eij", P, F) / J[:, None, None]
        scale = (np.einsum("eik,ejk->eij", ref["P_abs"], aF) / np.abs(J)[:, None, None]).max()
        _assert_le(f"recover cauchy_stress {tag}", np.abs(got["cauchy_stress"] - sig).max(), scale)
        if d == 3:
            dev = sig - np.einsum("ekk->e", sig)[:, None, None] / 3 * I
            vm = np.sqrt(LD(1.5) * np.einsum("eij,eij->e", dev, dev))
        else:
            vm = np.sqrt(sig[:, 0, 0] ** 2 - sig[:, 0, 0] * sig[:, 1, 1] + sig[:, 1, 1] ** 2 + 3 * sig[:, 0, 1] ** 2)
        # von Mises is a seminorm of sigma with Lipschitz constant sqrt(3/2) * 3 < 3.7 in the largest entry
        _assert_le(f"recover von_mises {tag}", np.abs(got["von_mises"] - vm).max(), 3.7 * scale)
        out += [got["cauchy_stress"], got["von_mises"]]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("variant,case", GPU_CASES)
def test_stable_neo_hookean_against_long_double(variant, case):
    kind, m, w, p = mesh_of(variant)
    d = m.vertices.shape[1]
    u = deformation(case, m.vertices, m.connectivity)
    ref = reference(kind, m, w, p, u, case)
    lame = params_of(case, d)
    tag = f"{variant} ({case}) {OP}"
    eng = fa.Engine(0)
    try:
        asm = _builder(eng, m, _table(w, p, lame), u)
        x = np.random.default_rng(7).standard_normal(len(u))
        ks = tld._assembled_routes(eng, asm, kind, OP, ref, tag)
        ks.update(_mask_and_reproducible(eng, asm, kind, ref, tag))
        y, dg = tld._tangent_route(eng, asm, kind, ref, x, tag)
        outs = list(ks.values()) + [y, dg]
        if variant in ("HEX8_AFFINE", "HEX8_GENERAL", "TET10"):
            tld._shifted_route(eng, asm, kind, ref, x, tag)
        r, e = tld._vector_routes(eng, asm, kind, ref, case, tag)
        outs += [r, np.array([e])] + _recovery(eng, kind, m, p, u, lame, case, tag)
        for o in outs:   # (cases f, g, h are the point: nothing NaN or inf through inversion; an unfinished element would have raised)
            assert np.isfinite(o).all()
        if case != "e":
            return
        # rotation invariance on the device alone: K(u_R) = P K(0) P^T, T(u_R) x = P T(0) P^T x, diag likewise; r(u_R) = 0 = psi(u_R)
        R = F3["e"] if d == 3 else F2["e"]
        idx, sign = tld._block_perm(R, m.num_nodes())
        ref0 = reference(kind, m, w, p, np.zeros_like(u), "e")
        eng.set_u(np.zeros_like(u))
        ks0 = tld._assembled_routes(eng, asm, kind, OP, ref0, f"{variant} (0) {OP}")
        for route, k0v in ks0.items():
            k0 = tld.k_rotated_from(k0v, ref0, idx, sign)
            _assert_le(f"rotation K {route} {kind} {OP}", np.abs(ks[route] - k0).max(), np.abs(k0).max())
        xt = np.empty_like(x)
        xt[idx] = sign * x
        y0 = np.empty_like(x)
        fa.MatrixFreeTangent(asm).apply(y0, xt)
        _, bound = ref0.apply(xt)
        _assert_le(f"rotation apply {kind} {OP}", np.abs(y - sign * y0[idx]).max(), bound)
        d0 = fa.MatrixFreeTangent(asm).diagonal()
        _assert_le(f"rotation diag {kind} {OP}", np.abs(dg - d0[idx]).max(), np.abs(d0).max())
        _assert_le(f"rotation residual {kind} {OP}", np.abs(r).max(), ref.residual_scale(terms=True).max())
        _assert_le(f"rotation energy {kind} {OP}", abs(e), ref.energy_scale(terms=True))
    finally:
        eng.close()


@pytest.mark.gpu
def test_per_point_parameters_through_a_compact_table():
    """three rules of parameters that differ from point to point, elements dealt round robin: K, tangent, residual and energy"""
    kind, m, w, p = mesh_of("TET4")
    u = deformation("a", m.vertices)
    nq, E = len(w), m.num_elements()
    lm = params_of("a", 3)
    per_point = np.stack([lm.mu * (1.0 + 0.25 * np.arange(nq) / nq), lm.lambda_ * (1.0 - 0.3 * np.arange(nq) / nq)], axis=1)
    rules = np.stack([per_point * f for f in (1.0, 1.7, 0.6)])
    e2r = np.arange(E, dtype=np.uint64) % 3
    ref = snh.Reference(kind, m.vertices, m.connectivity, w, p, u, lm.mu, lm.lambda_, rho=RHO, per_point=rules[e2r.astype(np.int64)])
    uniform = reference(kind, m, w, p, u, "a")
    assert np.abs(ref.ke - uniform.ke).max() > 1e-2 * np.abs(uniform.ke).max()
    tag = f"TET4 (a) compact {OP}"
    eng = fa.Engine(0)
    try:
        qt = fa.CompactQuadratureTable(p, w, [[tuple(x) for x in r] for r in rules], e2r)
        asm = _builder(eng, m, qt, u)
        tld._check_k(f"K {tag}", fa.CsrAssembler(fa.SCATTER_GATHER).assemble(asm), ref)
        x = np.random.default_rng(7).standard_normal(len(u))
        y = np.full(len(x), np.nan)
        t = fa.MatrixFreeTangent(asm)
        t.apply(y, x)
        yh, bound = ref.apply(x)
        _assert_le(f"apply {tag}", np.abs(y - yh).max(), bound)
        _assert_le(f"diag {tag}", np.abs(t.diagonal() - ref.diagonal()).max(), np.abs(ref.diagonal()).max())
        r = fa.VectorAssembler().assemble_vector(asm)
        _assert_le(f"residual {tag}", np.abs(r - ref.residual()).max(), ref.residual_scale().max())
        _assert_le(f"energy {tag}", abs(fa.assemble_scalar(asm) - ref.energy()), ref.energy_scale())
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", tld.VARIANTS)
def test_linearisation_at_rest_is_the_device_linear_elastic_matrix(variant):
    """K(0) with converted parameters against the device's own LinearElastic K on the same mesh: no reference involved"""
    kind, m, w, p = mesh_of(variant)
    d = m.vertices.shape[1]
    u0 = np.zeros(m.vertices.size)
    eng = fa.Engine(0)
    try:
        k = _host(fa.CsrAssembler(fa.SCATTER_GATHER).assemble(_builder(eng, m, _table(w, p, tld.LAME.for_stable_neo_hookean(d)), u0)).values).copy()
        kl = _host(fa.CsrAssembler(fa.SCATTER_GATHER).assemble(_builder(eng, m, _table(w, p, tld.LAME), u0, fa.LinearElasticMaterial)).values)
        err = np.abs(k - kl).max() / np.abs(kl).max()
        print(f"{variant}: |K_snh(0) - K_le| / max|K| = {err:.3e}")
        assert err <= 1e-13
    finally:
        eng.close()


def _code(fn, *a, **kw):
    with pytest.raises(fa.FenrisError) as ei:
        fn(*a, **kw)
    return ei.value.code


@pytest.mark.gpu
def test_entry_points_and_error_codes():
    from fenris_amd import _ffi

    kind, m, w, p = mesh_of("TET10")
    u = deformation("a", m.vertices)
    eng = fa.Engine(0)
    try:
        assert eng._lib.fh_set_operator(eng._h, 8) == _ffi.FH_BAD_ARGUMENT and eng._lib.fh_set_operator(eng._h, -1) == _ffi.FH_BAD_ARGUMENT
        # no parameters: the law needs its (mu, lambda) like the other materials
        bare = fa.UniformQuadratureTable.from_points_and_weights(p, w)
        assert _code(lambda: fa.CsrAssembler(fa.SCATTER_GATHER).assemble(_builder(eng, m, bare, u))) == _ffi.FH_INVALID_STATE
        asm = _builder(eng, m, _table(w, p, params_of("a", 3)), u)
        # the operator-only entry points stay with the laws linear in u; the tangent's take it
        y = np.zeros(len(u))
        assert _code(fa.MatrixFreeOperator(asm).apply, y, np.ones(len(u))) == _ffi.FH_UNSUPPORTED
        fa.MatrixFreeTangent(asm).apply(y, np.ones(len(u)))
        assert np.isfinite(y).all() and np.any(y)
        # a shifted map without a density
        import torch
        xd, yd = torch.ones(len(u), dtype=torch.float64, device="cuda"), torch.zeros(len(u), dtype=torch.float64, device="cuda")
        fresh = fa.Engine(0)
        try:
            _builder(fresh, m, _table(w, p, params_of("a", 3)), u)
            rc = fresh._lib.fh_apply_shifted_tangent_dev(fresh._h, 1.0, 1.0, xd.data_ptr(), yd.data_ptr())
            assert rc == _ffi.FH_INVALID_STATE
        finally:
            fresh.close()
        # FH_TENSOR data under this operator is ignored by it; the mass operators and FH_TENSOR keep FH_UNSUPPORTED where they had it
        eng.set_operator(_ffi.TENSOR)
        assert _code(fa.VectorAssembler().assemble_vector, asm) in (_ffi.FH_UNSUPPORTED, _ffi.FH_INVALID_STATE)
        eng.set_operator(_ffi.MASS_VECTOR)
        assert _code(eng.recover, "stress_pk1", "points") == _ffi.FH_UNSUPPORTED
        # ragged connectivity is refused as for the others
        eng.set_connectivity_ragged(3, 5, np.array([0, 3, 5], dtype=np.uint64), np.array([0, 1, 2, 3, 4], dtype=np.uint64))
        assert _code(eng.set_operator, _ffi.STABLE_NEO_HOOKEAN) == _ffi.FH_INVALID_STATE
    finally:
        eng.close()


# ------------------------------------------------------------------------------------------------------------------ solvers
import scipy.sparse as sp

import dynamics_reference as dr

SOLVER_LAME = tld.LAME.for_stable_neo_hookean(3)
SOLVER_RHO = 1000.0


def _solver_mesh(kind):
    from fenris_amd import quadrature

    if kind == "TET4":
        return fa.procedural.create_unit_box_uniform_tet_mesh_3d(3), *map(np.asarray, quadrature.total_order.tetrahedron(2))
    return fa.procedural.create_rectangular_uniform_hex_mesh(0.25, 4, 3, 3, 1), *map(np.asarray, quadrature.tensor.hexahedron_gauss(2))


def _clamp(m):
    x = m.vertices[:, 0]
    return np.where(np.isclose(x, x.min()))[0]


class Problem(dr.Problem):
    """dynamics_reference's problem on the long-double reference of this law: residual, energy, tangent and mass come from
    stable_neo_hookean_reference (rounded to double where the integrators take them over); perm: another order of the elements, so another
    summation order and nothing else"""

    def __init__(self, kind, m, w, p, f=None, perm=None, lame=SOLVER_LAME, rho=SOLVER_RHO):
        conn = np.asarray(m.connectivity)
        self.conn = conn if perm is None else conn[np.random.default_rng(perm).permutation(len(conn))]
        self.kind, self.vertices, self.w, self.p, self.lame, self.rho = kind, np.asarray(m.vertices), w, p, lame, rho
        self.d = self.s = self.vertices.shape[1]
        self.N = len(self.vertices)
        self.n = self.s * self.N
        self.free = np.ones(self.n, dtype=bool)
        for k in range(self.s):
            self.free[self.s * _clamp(m) + k] = False
        self.f = np.zeros(self.n) if f is None else np.asarray(f, dtype=np.float64).reshape(-1)
        self.load_factor, self.direct, self._mass = None, "sparse", None

    def ref(self, u):
        return snh.Reference(self.kind, self.vertices, self.conn, self.w, self.p, u, self.lame.mu, self.lame.lambda_, rho=self.rho)

    def residual(self, u):
        return self.ref(u).residual().astype(np.float64)

    def energy(self, u):
        return float(self.ref(u).energy())

    def _csr(self, ref, which):
        ro, ci = ref.pattern()
        return sp.csr_matrix((ref.csr_values(ro, ci, which).astype(np.float64), ci, ro), shape=(self.n, self.n))

    def tangent(self, u):
        return self._csr(self.ref(u), "K")

    def mass(self):
        if self._mass is None:
            self._mass = self._csr(self.ref(np.zeros(self.n)), "M")
        return self._mass


def _body_load(m, total):
    """a force `total` along +x spread evenly over the nodes off the clamped face"""
    f = np.zeros(3 * m.num_nodes())
    f[0::3] = total / m.num_nodes()
    f[3 * _clamp(m)] = 0.0
    return f


def _solver_assembler(engine, m, w, p, material=None, lame=SOLVER_LAME, u=None):
    return _builder(engine, m, _table(w, p, lame), np.zeros(3 * m.num_nodes()) if u is None else u, material)


# a body load along +x sized on the CPU reference (dynamics_reference.newton on Problem) so that the stretches reach about 1.3
NEWTON_LOAD = {"TET4": 5.0e5, "HEX8": 2.5e5, "HEX8_REFINED": 2.5e5}


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["TET4", "HEX8", "HEX8_REFINED"])
def test_newton_converges_to_the_reference_equilibrium(case):
    """MatrixFreeNewton, one face clamped, Jacobi-PCG on the two small meshes; on the uniform refinement of the Hex8 box (the box itself is the
    coarse level) multigrid-PCG.  The long-double residual at the returned u balances the load to the tolerance on the free dofs, and every
    point has det F > 0 there."""
    kind = case.split("_")[0]
    m, w, p = _solver_mesh(kind)
    eng = fa.Engine(0)
    try:
        mg = None
        if case == "HEX8_REFINED":
            coarse = m
            m, transfer = fa.refine_uniformly_with_transfer(coarse)
        f = _body_load(m, NEWTON_LOAD[case])
        asm = _solver_assembler(eng, m, w, p)
        solver = fa.MatrixFreeNewton(asm).with_dirichlet_nodes(_clamp(m)).with_load(f)
        if case == "HEX8_REFINED":
            mg = fa.GeometricMultigrid(asm, [coarse], [transfer])
            solver.with_multigrid(mg)
        tol = 1e-8 * np.linalg.norm(f)
        u = np.zeros_like(f)
        res = solver.solve(u, fa.NewtonSettings(30, tol), linear_rel_tol=1e-12)
        prob = Problem(kind, m, w, p, f)
        ref = prob.ref(u)
        defect = np.linalg.norm((ref.residual().astype(np.float64) - f)[prob.free])
        print(f"{case}: {res.iterations} Newton iterations, device ||F|| {res.residual_norm:.3e}, reference ||r(u) - f|| {defect:.3e} (tol {tol:.3e}), "
              f"det F in [{ref.det_F_min:.3f}, {ref.det_F_max:.3f}], largest displacement {np.abs(u).max():.3f}")
        assert res.residual_norm <= tol and res.linear_status == 0
        assert defect <= tol
        assert ref.det_F_min > 0.0 and ref.det_F_max > 1.15      # the tangent is definite at such states; the stretches are not small
        assert res.linear_iterations > 0
    finally:
        eng.close()


# d_perm (the reference against itself under another element order), and the tolerance max(20 d_perm [+ d_newton], 1e-13), measured on the CPU
# with the reference alone as test_dynamics.py measures its own; the tests measure them again and want them within a factor 10 of these
DYNAMICS_TOLERANCE = {"central_through_inversion": (6.5e-17, 0.0, 1.0e-13), "euler_one_step": (4.2e-16, 0.0, 1.0e-13)}
DT_FRACTION = 0.0625   # of stable_dt() at u = 0.  At 0.25 the reference's total energy moves by 9.4e-3 relative over the 16 steps (the start is
                       # far from rest), at 0.0625 by 5.9e-4: within the 1e-3 asked for


def _trajectory(x):
    return x[0], x[1], x[2], x[3]


@pytest.mark.gpu
def test_explicit_dynamics_run_through_inversion():
    """CentralDifference from the fully reflected state (f), lumped mass, no load: 16 steps with a record every 4 against
    dynamics_reference.central_difference on the long-double reference; det F changes sign on the way.  The same start with NeoHookean is
    FH_DYNAMICS_NONFINITE with no step done."""
    import test_dynamics as td
    from fenris_amd import _ffi

    kind = "TET4"
    m, w, p = _solver_mesh(kind)
    u0 = deformation("f", m.vertices)
    z = np.zeros_like(u0)
    eng = fa.Engine(0)
    try:
        asm = _solver_assembler(eng, m, w, p)
        ti = fa.CentralDifference(asm, SOLVER_RHO, 1.0).with_dirichlet_nodes(_clamp(m))
        ti.set_state(z)
        dt = DT_FRACTION * ti.stable_dt()[1]
        ti.close()
        prob = Problem(kind, m, w, p)
        ref = dr.central_difference(prob, u0, z, dt, 16, 4)
        total = ref[3][:, 0] + ref[3][:, 1]
        e0 = prob.energy(u0)
        assert all(np.isfinite(x).all() for x in ref) and np.abs(total - e0).max() <= 1e-3 * e0
        end = prob.ref(ref[0])
        assert prob.ref(u0).det_F_max < 0.0 and end.det_F_min < 0.0 < end.det_F_max
        d_perm = td._rel_diff(ref, dr.central_difference(Problem(kind, m, w, p, perm=7), u0, z, dt, 16, 4))
        tol = td._check_constants("central_through_inversion", d_perm, 0.0, max(20.0 * d_perm, 1e-13), DYNAMICS_TOLERANCE)
        ti = fa.CentralDifference(asm, SOLVER_RHO, dt).with_dirichlet_nodes(_clamp(m))
        ti.set_state(u0)
        rec = ti.step(16, record_every=4)
        assert rec.steps_done == 16 and len(rec.time) == 4
        u, v, a, _, step = ti.state()
        assert step == 16 and np.isfinite(u).all() and np.isfinite(v).all() and np.isfinite(a).all()
        td._assert_parity((u, v, a, td._records(rec)), _trajectory(ref), tol, "central difference through inversion")
        ti.close()
        # the contrast that is the point of the law
        nh = fa.CentralDifference(_solver_assembler(eng, m, w, p, fa.NeoHookeanMaterial, tld.LAME), SOLVER_RHO, dt).with_dirichlet_nodes(_clamp(m))
        nh.set_state(u0)
        with pytest.raises(fa.DynamicsError) as ei:
            nh.step(16)
        assert ei.value.code == _ffi.FH_DYNAMICS_NONFINITE and ei.value.steps_done == 0
    finally:
        eng.close()


@pytest.mark.gpu
def test_one_backward_euler_step_from_a_large_strain():
    """one implicit step from the state (a) on the Hex8 box against dynamics_reference.implicit on the long-double reference"""
    import test_dynamics as td

    kind = "HEX8"
    m, w, p = _solver_mesh(kind)
    u0 = deformation("a", m.vertices)
    z = np.zeros_like(u0)
    dt = 5.0e-3        # about 0.8 of the explicit limit of this box: mass and stiffness both matter in M + dt^2 K
    prob = Problem(kind, m, w, p)
    r0 = prob.residual(u0)
    r0[~prob.free] = 0.0
    tol_n = 1e-10 * dt * dt * np.linalg.norm(r0)

    def run(pr, t):
        st, u, v, a, rec, done, _ = dr.implicit(pr, "euler", u0, z, dt, 1, 0, tol=t)
        assert st == "ok" and done == 1
        return u, v, a, rec

    ref = run(prob, tol_n)
    d_perm = td._rel_diff(ref, run(Problem(kind, m, w, p, perm=7), tol_n))
    d_newton = td._rel_diff(ref, run(prob, tol_n / 100.0))
    tol = td._check_constants("euler_one_step", d_perm, d_newton, max(20.0 * (d_perm + d_newton), 1e-13), DYNAMICS_TOLERANCE)
    eng = fa.Engine(0)
    try:
        ti = fa.BackwardEuler(_solver_assembler(eng, m, w, p), SOLVER_RHO, dt).with_dirichlet_nodes(_clamp(m))
        ti.with_newton(fa.NewtonSettings(30, tol_n), linear_rel_tol=1e-12)
        ti.set_state(u0)
        rec = ti.step(1)
        assert rec.steps_done == 1
        u, v, a, _, step = ti.state()
        td._assert_parity((u, v, a, td._records(rec)), ref, tol, "backward Euler, one step from (a)")
        assert np.abs(u - u0).max() > 0.1
    finally:
        eng.close()


@pytest.mark.gpu
def test_eigenmodes_at_rest_are_linear_elasticity():
    """MatrixFreeEigensolver at u = 0 with converted parameters returns the LinearElastic eigenvalues of the same mesh"""
    m, w, p = _solver_mesh("HEX8")
    tol = 1e-8
    eng = fa.Engine(0)
    try:
        values = {}
        for name, material, lame in (("le", fa.LinearElasticMaterial, tld.LAME), ("snh", fa.StableNeoHookeanMaterial, SOLVER_LAME)):
            asm = _solver_assembler(eng, m, w, p, material, lame)
            res = fa.MatrixFreeEigensolver(asm, SOLVER_RHO).with_dirichlet_nodes(_clamp(m)).solve(4, tol=tol)
            values[name] = np.asarray(res.values)
        err = np.abs(values["snh"] - values["le"]) / values["le"]
        print("eigenvalues", values["le"], "relative difference", err)
        assert (values["le"] > 0).all() and err.max() <= tol
    finally:
        eng.close()
