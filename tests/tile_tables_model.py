"""A model of the element-tile tables (fenris_amd/csrc/vector_tiles.hip) in numpy, and the meshes that put chosen corners of those tables
under a kernel.  A helper for tests, not a conftest.

The tables: the elements are sorted by the Morton key of their centroids (a stable radix sort) and cut into tiles of 256; a tile leaves one
partial sum per DISTINCT node of its elements, and every node owns the list of its partials, one per tile that touches it.  When all
vertices coincide every key is 0, the stable sort keeps the element order, and TILE t IS EXACTLY THE ELEMENTS [256 t, 256 t + 256): the
tables then follow from the connectivity alone, which is what `tables` computes.  fh_update_vertices keeps the tables, so a mesh handed over
with all vertices zero, its tables built (fh_vector_tiles_stats builds them), and then given its true coordinates is valid geometry on
tiles this model predicts.  With the element order dealt at random such a tile's nodes are scattered over the whole mesh: `dealt`.

For a mesh handed over with its true coordinates the tiles follow the Morton order, which is not modelled: only the number of tiles and
partials <= E n hold -- except for a soup, where every element has its own nodes and every partition into tiles gives the same counts."""
from types import SimpleNamespace

import numpy as np

import fenris_amd as fa

TILE = 256


def tables(connectivity, num_nodes, tile=TILE):
    """tiles T, partials P, tile_nodes (T,): distinct nodes per tile, list_len (num_nodes,): partials per node, and the two maxima, for
    tiles of consecutive elements"""
    conn = np.asarray(connectivity).astype(np.int64)
    E, n = conn.shape
    T = (E + tile - 1) // tile
    pairs = np.unique(np.repeat(np.arange(E) // tile, n) * num_nodes + conn.reshape(-1))   # (tile, node), each once
    tile_nodes = np.bincount(pairs // num_nodes, minlength=T)
    list_len = np.bincount(pairs % num_nodes, minlength=num_nodes)
    return SimpleNamespace(tiles=T, partials=len(pairs), tile_nodes=tile_nodes, list_len=list_len, max_tile_nodes=int(tile_nodes.max()),
                           max_node_partials=int(list_len.max()), elements=E, nodes_per_element=n)


def stats(model):
    """what Engine.vector_tiles_stats() returns for these tables"""
    return model.tiles, model.partials, model.max_tile_nodes, model.max_node_partials


def dealt(mesh, seed):
    """the mesh with its elements in a random order (the nodes keep their numbers)"""
    perm = np.random.default_rng(seed).permutation(mesh.num_elements())
    return fa.Mesh(mesh.vertices, np.asarray(mesh.connectivity)[perm], mesh.elem_kind)


def collapsed(mesh):
    """the same connectivity with every vertex at the origin: all centroids coincide, the tiles are consecutive runs of elements"""
    return fa.Mesh(np.zeros_like(mesh.vertices), mesh.connectivity, mesh.elem_kind)


def soup(mesh, front, back):
    """every element gets its own copies of its vertices, with `front` unused vertices in front of them and `back` behind"""
    conn = np.asarray(mesh.connectivity).astype(np.int64)
    d = mesh.vertices.shape[1]
    verts = np.concatenate([np.zeros((front, d)), mesh.vertices[conn.reshape(-1)], np.zeros((back, d))])
    return fa.Mesh(verts, (front + np.arange(conn.size).reshape(conn.shape)).astype(np.uint64), mesh.elem_kind)


def soup_tables(mesh, tile=TILE):
    """the tables of a soup, whatever order its tiles take the elements in: every (element, local node) entry is a partial of its own"""
    E, n = np.asarray(mesh.connectivity).shape
    used = np.zeros(mesh.num_nodes(), dtype=np.int64)
    used[np.asarray(mesh.connectivity).astype(np.int64).reshape(-1)] = 1
    assert used.sum() == E * n, "not a soup"
    T = (E + tile - 1) // tile
    tile_nodes = np.full(T, tile * n)
    tile_nodes[-1] = (E - (T - 1) * tile) * n
    return SimpleNamespace(tiles=T, partials=E * n, tile_nodes=tile_nodes, list_len=used, max_tile_nodes=int(tile_nodes.max()),
                           max_node_partials=1, elements=E, nodes_per_element=n)


def first_elements(mesh, E):
    """the first E elements of a mesh; the nodes that drop out stay, as nodes without elements"""
    return fa.Mesh(mesh.vertices, np.asarray(mesh.connectivity)[:E], mesh.elem_kind)


def unused_nodes(mesh):
    used = np.zeros(mesh.num_nodes(), dtype=bool)
    used[np.asarray(mesh.connectivity).astype(np.int64).reshape(-1)] = True
    return np.nonzero(~used)[0]


# ---- the meshes of tests/test_tile_corners.py: name -> (kind, mesh with its true coordinates, dealt?, model of its tables or None)
def _jitter(mesh, amount, seed):
    """every vertex moved by up to `amount` (a fraction of the unit cell edge) in every coordinate: no element stays affine"""
    rng = np.random.default_rng(seed)
    return fa.Mesh(mesh.vertices + amount * rng.uniform(-1, 1, mesh.vertices.shape), mesh.connectivity, mesh.elem_kind)


def _tri_of(quad):
    c = np.asarray(quad.connectivity)
    return fa.Mesh(quad.vertices, np.ascontiguousarray(np.stack([c[:, [0, 1, 2]], c[:, [0, 2, 3]]], axis=1).reshape(-1, 3)), fa.TRI3)


_CASES = {}


def corner_cases():
    """built once: {name: SimpleNamespace(name, kind, mesh, dealt, model, natural_tiles)}"""
    if _CASES:
        return _CASES
    P = fa.procedural

    def add(name, kind, mesh, is_dealt=False, is_soup=False):
        model = tables(mesh.connectivity, mesh.num_nodes()) if is_dealt else soup_tables(mesh) if is_soup else None
        _CASES[name] = SimpleNamespace(name=name, kind=kind, mesh=mesh, dealt=is_dealt, model=model,
                                       natural_tiles=(mesh.num_elements() + TILE - 1) // TILE)

    hexbox = P.create_rectangular_uniform_hex_mesh(1.0, 13, 13, 13, 1)                # 2197 elements: 9 tiles, the last ragged
    add("hex8 dealt", "HEX8", dealt(_jitter(hexbox, 0.03, 1), 101), is_dealt=True)
    add("hex8 dealt affine", "HEX8", dealt(hexbox, 102), is_dealt=True)               # every element a cube: MONO = 2, the moment form
    add("tet4 dealt", "TET4", dealt(_jitter(P.create_rectangular_uniform_tet_mesh(1.0, 6, 6, 6, 1), 0.03, 2), 103), is_dealt=True)   # 2592: 11 tiles
    quad = P.create_rectangular_uniform_quad_mesh_2d(1.0, 40, 40, 1, (0.0, 40.0))
    add("quad4 dealt", "QUAD4", dealt(_jitter(quad, 0.03, 3), 104), is_dealt=True)   # 1600: 7 tiles
    tri = _tri_of(P.create_rectangular_uniform_quad_mesh_2d(1.0, 28, 28, 1, (0.0, 28.0)))
    add("tri3 dealt", "TRI3", dealt(_jitter(tri, 0.03, 4), 105), is_dealt=True)      # 1568: 7 tiles
    # soups: 2048 / 1024 distinct nodes in a full tile; 2560 / 3072 used nodes, with the unused ones N = 1 and N = 0 (mod 256)
    hs = _jitter(P.create_rectangular_uniform_hex_mesh(1.0, 8, 8, 5, 1), 0.03, 5)
    add("hex8 soup N=1", "HEX8", soup(hs, 2, 255), is_soup=True)
    add("hex8 soup N=0", "HEX8", soup(hs, 3, 253), is_soup=True)
    tets = _jitter(P.create_rectangular_uniform_tet_mesh(1.0, 4, 4, 4, 1), 0.03, 6)
    add("tet4 soup N=1", "TET4", soup(tets, 2, 255), is_soup=True)
    add("tet4 soup N=0", "TET4", soup(tets, 3, 253), is_soup=True)
    # the tile count against 8 (the eight XCD shares of the grid) and a tile of one element
    base = _jitter(P.create_rectangular_uniform_quad_mesh_2d(1.0, 64, 33, 1, (0.0, 33.0)), 0.03, 7)
    for E in (256, 257, 2048, 2049):
        add(f"quad4 first {E}", "QUAD4", first_elements(base, E))
    return _CASES
