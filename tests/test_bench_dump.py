"""bench.py --dump-outputs DIR: what the last timed step computed (the CSR values of K) as float64 .npy files, every entry or a fixed
seeded sample, the same from run to run -- so that two builds can be compared output for output.  The sampling on the host (CPU); the
dump of a real run against the oracle (GPU)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Pattern:
    """stands in for the engine: CSR row offsets of `rows` rows of `per_row` entries"""

    def __init__(self, rows, per_row):
        self.ro = (per_row * np.arange(rows + 1)).astype(np.uint64)

    def pattern(self, want_cols=True):
        assert not want_cols
        return self.ro, None


def _load(d, prefix=""):
    return {n: np.load(os.path.join(d, f"{prefix}{n}.npy")) for n in ("values", "entry", "row")}


def test_dump_writes_every_entry_of_a_small_array(tmp_path):
    torch = pytest.importorskip("torch")
    b = _bench()
    vals = torch.arange(60, dtype=torch.float64) * 0.5
    b.dump_outputs(str(tmp_path), _Pattern(12, 5), vals, 0, 1, np, torch)
    out = _load(str(tmp_path))
    assert all(a.dtype == np.float64 for a in out.values())
    assert np.array_equal(out["entry"], np.arange(60))
    assert np.array_equal(out["values"], vals.numpy())
    assert np.array_equal(out["row"], np.arange(60) // 5)


def test_dump_samples_a_large_array_the_same_way_every_time(tmp_path, monkeypatch):
    torch = pytest.importorskip("torch")
    b = _bench()
    monkeypatch.setattr(b, "DUMP_ENTRIES", 256)
    nnz = 7 * 3001
    vals = torch.randn(nnz, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    runs = []
    for i in range(2):
        d = str(tmp_path / str(i))
        b.dump_outputs(d, _Pattern(3001, 7), vals, 0, 1, np, torch)
        runs.append(_load(d))
    e = runs[0]["entry"].astype(np.int64)
    assert 0 < len(e) <= 256 and np.all(np.diff(e) > 0) and e[-1] < nnz
    assert np.array_equal(runs[0]["values"], vals.numpy()[e])
    assert np.array_equal(runs[0]["row"], e // 7)
    for n in ("values", "entry", "row"):
        assert np.array_equal(runs[0][n], runs[1][n]), n


def test_dump_ranks_share_the_budget(tmp_path):
    torch = pytest.importorskip("torch")
    b = _bench()
    nnz = b.DUMP_ENTRIES   # more than one rank's share
    b.dump_outputs(str(tmp_path), _Pattern(nnz // 8, 8), torch.ones(nnz, dtype=torch.float64), 1, 4, np, torch)
    out = _load(str(tmp_path), "rank1_")
    assert len(out["entry"]) <= b.DUMP_ENTRIES // 4
    assert not os.path.exists(os.path.join(str(tmp_path), "values.npy"))


def test_dump_budget_is_under_64_mb():
    b = _bench()
    header = 128   # one .npy header of a 1-D array
    assert 3 * (8 * b.DUMP_ENTRIES + header) <= 64 * 10**6


def test_steps_below_one_are_refused():
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0", "--no-traffic"], capture_output=True, text=True,
                        timeout=120)
    assert pr.returncode == 2 and "--steps" in pr.stderr


@pytest.mark.gpu
def test_dump_of_a_bench_run_is_the_oracle_matrix_and_repeats(tmp_path, oracle):
    """two runs of the headline path on a 6^3 box: the dumps agree bit for bit and hold K of the oracle, every entry"""
    import fenris_amd as fa
    from fenris_amd import quadrature

    cells = 6
    dirs = [str(tmp_path / f"run{i}") for i in range(2)]
    for d, steps in zip(dirs, (2, 3)):
        pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "ns", "--cells", str(cells),
                             "--steps", str(steps), "--warmup", "1", "--no-cpu-baseline", "--no-traffic", "--no-secondary", "--no-settle",
                             "--dump-outputs", d], capture_output=True, text=True, timeout=600)
        assert pr.returncode == 0, pr.stderr[-3000:]
        line = json.loads([ln for ln in pr.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["steps"] == steps and line["roofline"]["kernel"] == "k_affine_rows"
    a, b = _load(dirs[0]), _load(dirs[1])
    for n in ("values", "entry", "row"):
        assert np.array_equal(a[n], b[n]), n

    mesh = fa.procedural.create_rectangular_uniform_hex_mesh(1.0, 1, 1, 1, cells)
    w, p = quadrature.tensor.hexahedron_gauss(2)
    lame = fa.LameParameters.from_young_poisson(fa.YoungPoisson(1e6, 0.2))
    ref = oracle.ElementAssembler(oracle.HEX8, oracle.LINEAR_ELASTIC, mesh.vertices, mesh.connectivity, w, p, params=lame.as_pair())
    st, _, ro, _, vals = oracle.assemble(ref)
    assert st == 0
    assert np.array_equal(a["entry"], np.arange(len(vals)))
    assert np.array_equal(a["row"], np.repeat(np.arange(len(ro) - 1), np.diff(ro.astype(np.int64))))
    assert np.abs(a["values"] - vals).max() <= 1e-12 * np.abs(vals).max()
