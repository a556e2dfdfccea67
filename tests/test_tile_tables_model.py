"""No GPU: the model of the element-tile tables (tile_tables_model.py) shows, on the meshes of test_tile_corners.py, every regime those tests
aim at; the LAPLACE model and the per-element density of the long-double reference (hp_reference.py) against the oracle; the stats entry
point is declared everywhere."""
import os

import numpy as np
import pytest

import fenris_amd as fa
import hp_reference as hp
import tile_tables_model as ttm
from fenris_amd import _ffi, quadrature

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tables_of_a_hand_counted_connectivity():
    """tiles of two elements: {0,1,2},{2,3,4} | {0,4,5},{5,6,0} | {2,2,2}; node 7 has no element"""
    conn = np.array([[0, 1, 2], [2, 3, 4], [0, 4, 5], [5, 6, 0], [2, 2, 2]])
    m = ttm.tables(conn, 8, tile=2)
    assert ttm.stats(m) == (3, 5 + 4 + 1, 5, 2)
    assert m.tile_nodes.tolist() == [5, 4, 1]
    assert m.list_len.tolist() == [2, 1, 2, 1, 2, 1, 1, 0]


def test_the_meshes_show_every_regime():
    cases = ttm.corner_cases()
    lens = set()
    for c in cases.values():
        if c.model is not None:
            lens |= set(np.unique(c.model.list_len).tolist())
            assert c.model.tiles == c.natural_tiles and c.model.partials <= c.mesh.num_elements() * c.model.nodes_per_element
    # a node without elements, one partial, a full group of four, one more than a group (the clamp of the last group), two full groups,
    # a third group
    assert {0, 1, 4, 5, 8, 9} <= lens, sorted(lens)
    # more than 2 x 256 distinct nodes in a tile: the loop of TileSums::sum past the two preloaded starts, with the entries in LDS (N = 8, 4)
    # and read from global memory (N = 3)
    for kind in ("HEX8", "TET4", "TRI3"):
        assert max(c.model.max_tile_nodes for c in cases.values() if c.kind == kind and c.model is not None) > 512, kind
    h, t, tri, q = cases["hex8 dealt"].model, cases["tet4 dealt"].model, cases["tri3 dealt"].model, cases["quad4 dealt"].model
    assert h.max_node_partials == 8 and h.tile_nodes.min() > 512 and (h.list_len >= 5).sum() > 100
    assert cases["hex8 dealt affine"].model.max_node_partials == 8
    assert t.max_node_partials >= 9 and (t.list_len >= 9).sum() > 100
    assert tri.max_node_partials >= 5 and q.max_tile_nodes > 512
    assert cases["hex8 soup N=1"].model.max_tile_nodes == 2048 and cases["tet4 soup N=1"].model.max_tile_nodes == 1024
    # the node count against the 256 threads of a node pass's workgroup: one live thread in the last one, and a full last one; unused nodes
    # in front and behind
    for name, rem in (("hex8 soup N=1", 1), ("hex8 soup N=0", 0), ("tet4 soup N=1", 1), ("tet4 soup N=0", 0)):
        c = cases[name]
        assert c.mesh.num_nodes() % 256 == rem
        unused = ttm.unused_nodes(c.mesh)
        assert unused[0] == 0 and unused[-1] == c.mesh.num_nodes() - 1
    # the tile count against the eight shares of the element pass's grid; a tile of one element
    assert [cases[f"quad4 first {E}"].natural_tiles for E in (256, 257, 2048, 2049)] == [1, 2, 8, 9]
    assert all(len(ttm.unused_nodes(cases[f"quad4 first {E}"].mesh)) > 0 for E in (256, 257, 2048, 2049))
    # dealt: a tile's nodes are spread over the whole id range
    conn = np.asarray(cases["hex8 dealt"].mesh.connectivity).astype(np.int64)
    assert conn[:256].max() - conn[:256].min() > 0.9 * cases["hex8 dealt"].mesh.num_nodes()


def _small(kind):
    P = fa.procedural
    rng = np.random.default_rng(17)
    if kind == "HEX8":
        m, rule = P.create_rectangular_uniform_hex_mesh(1.0, 3, 2, 2, 1), quadrature.tensor.hexahedron_gauss(2)
    elif kind == "TET4":
        m, rule = P.create_rectangular_uniform_tet_mesh(1.0, 2, 1, 1, 1), quadrature.total_order.tetrahedron(2)
    elif kind == "QUAD4":
        m, rule = P.create_rectangular_uniform_quad_mesh_2d(1.0, 4, 3, 1, (0.0, 3.0)), quadrature.tensor.quadrilateral_gauss(2)
    else:
        m, rule = ttm._tri_of(P.create_rectangular_uniform_quad_mesh_2d(1.0, 4, 3, 1, (0.0, 3.0))), quadrature.total_order.triangle(2)
    m = fa.Mesh(m.vertices + 0.05 * rng.uniform(-1, 1, m.vertices.shape), m.connectivity, m.elem_kind)
    return m, np.asarray(rule[0]), np.asarray(rule[1])


@pytest.mark.parametrize("kind", ["HEX8", "TET4", "QUAD4", "TRI3"])
def test_laplace_reference_and_element_density_against_the_oracle(oracle, kind):
    m, w, p = _small(kind)
    rng = np.random.default_rng(3)
    E, N = m.num_elements(), m.num_nodes()
    u = rng.standard_normal(N)
    rho = 1.0 + rng.random(E)
    ref = hp.Reference(kind, "LAPLACE", m.vertices, m.connectivity, w, p, u, 0.0, 0.0, rho=rho)
    assert ref.s == 1 and ref.ndof == N
    okind = getattr(oracle, kind)
    oasm = oracle.ElementAssembler(okind, oracle.LAPLACE, m.vertices, m.connectivity, w, p, u=u)
    st, _, ro, ci, vals = oracle.assemble(oasm)
    assert st == 0
    k = ref.csr_values(ro, ci).astype(np.float64)
    assert np.abs(k - vals).max() <= 1e-13 * np.abs(vals).max()
    st, _, r = oracle.assemble_vector(oasm)
    assert st == 0 and np.abs(ref.residual().astype(np.float64) - r).max() <= 1e-13 * np.abs(r).max()
    st, _, e = oracle.assemble_scalar(oasm)
    assert st == 0 and abs(float(ref.energy()) - e) <= 1e-13 * abs(e)
    # K x and the diagonal are those of the assembled matrix
    x = rng.standard_normal(N)
    y, bound = ref.apply(x)
    import scipy.sparse as sp

    ks = sp.csr_matrix((vals, ci.astype(np.int64), ro.astype(np.int64)), shape=(N, N))
    assert np.abs(y.astype(np.float64) - ks @ x).max() <= 1e-13 * bound
    assert np.abs(ref.diagonal().astype(np.float64) - ks.diagonal()).max() <= 1e-13 * np.abs(ks.diagonal()).max()
    # the mass with one density per element: the oracle's scalar mass with one rule per element
    rp = np.zeros((E, len(w), 2))
    rp[:, :, 0] = rho[:, None]
    masm = oracle.ElementAssembler(okind, oracle.MASS_SCALAR, m.vertices, m.connectivity, w, p, elem_to_rule=np.arange(E), rule_params=rp)
    st, _, ro2, ci2, mv = oracle.assemble(masm)
    assert st == 0
    mm = ref.csr_values(ro2, ci2, which="M").astype(np.float64)
    assert np.abs(mm - mv).max() <= 1e-13 * np.abs(mv).max()
    # ... and the same density on a vector-valued model: the blocks are rho_e m_ab I
    d = m.vertices.shape[1]
    ref3 = hp.Reference(kind, "LINEAR_ELASTIC", m.vertices, m.connectivity, w, p, np.zeros(d * N), 1.0, 1.0, rho=rho)
    assert np.array_equal(ref3.me.reshape(E, ref.n, d, ref.n, d)[:, :, 0, :, 0], ref.me)
    assert np.array_equal(ref3.me.reshape(E, ref.n, d, ref.n, d)[:, :, 1, :, 1], ref.me)
    assert not ref3.me.reshape(E, ref.n, d, ref.n, d)[:, :, 0, :, 1].any()
    # one value for the whole mesh is still accepted, as a scalar and as an array of one
    one = hp.Reference(kind, "LAPLACE", m.vertices, m.connectivity, w, p, u, 0.0, 0.0, rho=np.array([2.5]))
    two = hp.Reference(kind, "LAPLACE", m.vertices, m.connectivity, w, p, u, 0.0, 0.0, rho=2.5)
    assert np.array_equal(one.me, two.me)


def test_stats_entry_point_is_declared():
    hdr = open(os.path.join(ROOT, "include", "fenris_hip.h")).read()
    rs = open(os.path.join(ROOT, "bindings", "fenris_hip_sys.rs")).read()
    name = "fh_vector_tiles_stats"
    assert name + "(" in hdr and name in _ffi.exported_symbols() and name in rs
    assert getattr(_ffi.lib(), name) is not None and hasattr(fa.Engine, "vector_tiles_stats")
