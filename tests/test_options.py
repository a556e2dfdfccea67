"""The FENRIS_HIP_* switches as one typed table (fenris_amd/csrc/options.def -> options.hpp -> fh_ctx::opt): the table against the sources
(no GPU: the names come through fh_option_name, the files are read as text) and the two readings through fh_set_option on a device."""
import ctypes as C
import glob
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fenris_amd", "csrc")
NAME = re.compile(r"FENRIS_HIP_[A-Z0-9_]+")

# every switch the library reads: an addition or a removal is a diff of this list
SWITCHES = [
    "FENRIS_HIP_ABLATE",
    "FENRIS_HIP_AFFINE_DEPTH",
    "FENRIS_HIP_AFFINE_GRID",
    "FENRIS_HIP_AFFINE_PRIO",
    "FENRIS_HIP_AFFINE_RECORDS_ALWAYS",
    "FENRIS_HIP_AFFINE_SHARED",
    "FENRIS_HIP_AFFINE_SHARED_AFTER",
    "FENRIS_HIP_AFFINE_SHARED_MAX_LISTS",
    "FENRIS_HIP_AFFINE_SHARED_MAX_RECORDS",
    "FENRIS_HIP_AFFINE_WGS_PER_CU",
    "FENRIS_HIP_EIGS_PROFILE",
    "FENRIS_HIP_GATHER_LDS_KB",
    "FENRIS_HIP_GATHER_MB",
    "FENRIS_HIP_GATHER_NB",
    "FENRIS_HIP_HEX27_NO_LEX",
    "FENRIS_HIP_HEX27_WGS_PER_CU",
    "FENRIS_HIP_HEX8_PRIO",
    "FENRIS_HIP_HOST_CUT",
    "FENRIS_HIP_NODE_ORDER",
    "FENRIS_HIP_NO_AFFINE",
    "FENRIS_HIP_NO_AFFINE_PASS",
    "FENRIS_HIP_NO_ELEMENT_PASS",
    "FENRIS_HIP_NO_ELEM_PAR",
    "FENRIS_HIP_NO_FAST",
    "FENRIS_HIP_NO_HEX8_ROWS",
    "FENRIS_HIP_NO_LANE_DEDUPE",
    "FENRIS_HIP_NO_LANE_TUNING",
    "FENRIS_HIP_NO_MFMA",
    "FENRIS_HIP_NO_MOMENT_RESIDUAL",
    "FENRIS_HIP_NO_MONOMIAL",
    "FENRIS_HIP_NO_NODE_ORDER",
    "FENRIS_HIP_NO_PIPE",
    "FENRIS_HIP_NO_ROWS",
    "FENRIS_HIP_NO_SWEEP",
    "FENRIS_HIP_NO_TWO_PASS",
    "FENRIS_HIP_NO_VECTOR_TILES",
    "FENRIS_HIP_PIPE_GRID",
    "FENRIS_HIP_PIPE_JT",
    "FENRIS_HIP_PIPE_QC",
    "FENRIS_HIP_PIPE_WGS_PER_CU",
    "FENRIS_HIP_PLACEMENT_KEEP",
    "FENRIS_HIP_RCCL_LIB",
    "FENRIS_HIP_SPMV_WAVE_PER_NODE",
    "FENRIS_HIP_TET4_PRIO",
    "FENRIS_HIP_TRACE",
    "FENRIS_HIP_TUNE_AFTER",
    "FENRIS_HIP_TWO_PASS",
    "FENRIS_HIP_TWO_PASS_FULL",
    "FENRIS_HIP_TWO_PASS_GRID",
    "FENRIS_HIP_TWO_PASS_MAX_GB",
    "FENRIS_HIP_TWO_PASS_NODES_PER_WAVE",
    "FENRIS_HIP_TWO_PASS_ROWS_GRID",
    "FENRIS_HIP_TWO_PASS_XCD_CHUNK",
    "FENRIS_HIP_VECTOR_ATOMICS",
    "FENRIS_HIP_VEC_WGS_PER_CU",
    "FENRIS_HIP_VERBOSE",
]
# FENRIS_HIP_* words that are no switches of the library: the Python loader's variable, the header's include guard, and the name this file
# uses for "a switch nobody declared"
NOT_SWITCHES = {"FENRIS_HIP_LIB", "FENRIS_HIP_H", "FENRIS_HIP_NO_SUCH_SWITCH"}


def _table():
    from fenris_amd import _ffi

    lib = C.CDLL(_ffi.LIB_PATH)      # (no context, no device)
    lib.fh_option_name.restype = C.c_char_p
    lib.fh_option_name.argtypes = [C.c_int]
    out = []
    while lib.fh_option_name(len(out)) is not None:
        out.append(lib.fh_option_name(len(out)).decode())
    assert lib.fh_option_name(-1) is None and lib.fh_option_name(len(out) + 1) is None
    return out


def _kinds():
    """{full name: kind} as options.def declares them"""
    text = open(os.path.join(CSRC, "options.def")).read()
    return {"FENRIS_HIP_" + n: k for n, k in re.findall(r"^FH_OPT\((\w+), (\w+),", text, flags=re.M)}


def _csrc_sources():
    return sorted(f for f in glob.glob(os.path.join(CSRC, "*")) if os.path.splitext(f)[1] in (".hip", ".hpp", ".cpp", ".def", ".inc", "") and os.path.isfile(f))


def test_table_is_todays_set_of_switches():
    names = _table()
    assert names and len(set(names)) == len(names)
    assert all(n.startswith("FENRIS_HIP_") for n in names)
    assert set(names) == set(SWITCHES) and len(SWITCHES) == 56
    kinds = _kinds()
    assert list(kinds) == names                                  # the export walks options.def in its order
    assert set(kinds.values()) == {"FLAG", "INT", "ENV_ONLY"}
    assert [n for n, k in kinds.items() if k == "ENV_ONLY"] == ["FENRIS_HIP_RCCL_LIB"]


def test_every_name_in_the_sources_is_declared():
    declared = set(_table()) | NOT_SWITCHES
    files = _csrc_sources() + glob.glob(os.path.join(ROOT, "include", "*.h")) + glob.glob(os.path.join(ROOT, "tests", "**", "*.py"), recursive=True) + \
        glob.glob(os.path.join(ROOT, "fenris_amd", "*.py")) + glob.glob(os.path.join(ROOT, "scripts", "*.py"))
    assert len(files) > 100
    stray = {(os.path.relpath(f, ROOT), n) for f in files for n in NAME.findall(open(f, errors="replace").read()) if n not in declared}
    assert not stray, sorted(stray)


def test_every_declared_switch_is_read():
    code = "".join(open(f).read() for f in _csrc_sources() if f.endswith((".hip", ".hpp")))
    dead = [n for n, k in _kinds().items() if k != "ENV_ONLY" and not re.search(r"opt\." + n[len("FENRIS_HIP_"):] + r"\b", code)]
    assert not dead, dead


def test_no_reads_by_string_are_left():
    """the map's readers and the process's `environ` (the identifier, not the word "environment") live in options.cpp only; the one getenv
    of a switch is group.hip's"""
    for f in _csrc_sources():
        text, base = open(f).read(), os.path.basename(f)
        if base != "options.cpp":
            assert "env_int(" not in text and "->env(" not in text and not re.search(r"\benviron\b", text), base
        if base != "group.hip":
            assert 'getenv("FENRIS_HIP' not in text, base


# ---- on a device
def _hex8_elastic(eng, n, u=None):
    import fenris_amd as fa
    from fenris_amd import quadrature

    mesh = fa.procedural.create_unit_box_uniform_hex_mesh_3d(n)
    w, p = quadrature.tensor.hexahedron_gauss(2)
    qt = fa.UniformQuadratureTable.from_points_and_weights(p, w).with_uniform_data(fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.2)))
    eng.set_mesh(mesh)
    eng.set_operator(fa._ffi.LINEAR_ELASTIC)
    eng.set_quadrature_table(qt)
    eng.set_u(u)
    return mesh


def _matrix(eng):
    import torch

    import fenris_amd as fa

    v = torch.full((eng.build_pattern(),), -11.5, dtype=torch.float64, device="cuda:0")
    eng.assemble_matrix(v, fa.SCATTER_GATHER | fa.ASSEMBLE_OVERWRITE)
    return v


@pytest.mark.gpu
def test_set_option_refuses_undeclared_and_process_wide_names():
    import torch

    import fenris_amd as fa

    eng, fresh = fa.Engine(0), fa.Engine(0)
    try:
        with pytest.raises(fa.FenrisError, match="FENRIS_HIP_NO_SUCH_SWITCH"):
            eng.set_option("FENRIS_HIP_NO_SUCH_SWITCH", 1)
        with pytest.raises(fa.FenrisError, match="FENRIS_HIP_RCCL_LIB.*environment"):
            eng.set_option("FENRIS_HIP_RCCL_LIB", "x")
        _hex8_elastic(eng, 2)
        _hex8_elastic(fresh, 2)
        assert torch.equal(_matrix(eng), _matrix(fresh))         # the refused calls left the context as it was
    finally:
        eng.close()
        fresh.close()


@pytest.mark.gpu
def test_a_flag_is_set_by_any_value():
    import torch

    tiled, plain = "k_element_pass_tiled + k_vector_from_partials", "k_element_pass + k_vector_from_elements_soa"
    import fenris_amd as fa

    eng = fa.Engine(0)
    try:
        u = 0.004 * np.random.default_rng(3).standard_normal(3 * 27)
        _hex8_elastic(eng, 2, u)

        def residual(want_kernel):
            out = torch.zeros(3 * 27, dtype=torch.float64, device="cuda:0")
            eng.assemble_vector(out)
            assert eng.last_kernel_name() == want_kernel, eng.last_kernel_name()
            return out.cpu().numpy()

        first = residual(tiled)
        eng.set_option("FENRIS_HIP_NO_VECTOR_TILES", "0")        # "0" is a value: the flag is SET
        second = residual(plain)
        eng.set_option("FENRIS_HIP_NO_VECTOR_TILES", None)
        third = residual(tiled)
        scale = np.abs(first).max()
        assert scale > 0
        for a, b in ((first, second), (second, third), (first, third)):
            print("routes differ by", np.abs(a - b).max() / scale)
            assert np.abs(a - b).max() <= 1e-12 * scale           # the bound tests/test_vector_tiles.py holds either route to
    finally:
        eng.close()


@pytest.mark.gpu
def test_an_int_is_its_value_and_empty_is_unset():
    import fenris_amd as fa

    eng = fa.Engine(0)
    try:
        eng.set_option("FENRIS_HIP_AFFINE_SHARED_AFTER", "0")    # the tables in the first sweep of the mesh
        _hex8_elastic(eng, 4)
        eng.set_option("FENRIS_HIP_AFFINE_SHARED", None)
        _matrix(eng)
        assert eng.last_kernel_name() == "k_affine_rows" and eng.affine_shared_stats()["shared"], eng.affine_shared_stats()
        eng.set_option("FENRIS_HIP_AFFINE_SHARED", "0")
        _matrix(eng)
        st = eng.affine_shared_stats()
        assert not st["shared"] and "FENRIS_HIP_AFFINE_SHARED=0" in st["reason"], st
        eng.set_option("FENRIS_HIP_AFFINE_SHARED", "")           # empty: unset, the default of elasticity (1)
        _matrix(eng)
        assert eng.affine_shared_stats()["shared"], eng.affine_shared_stats()
    finally:
        eng.close()
