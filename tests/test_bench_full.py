"""bench.py without --full does what its headline figure needs and nothing else; --full adds what takes runs of its own (HBM traffic by
PMC child passes, the plain fill, the CPU baseline, residual / energy and the other configurations).  The option on the host (CPU); a plain
and a --full run of the headline configuration at its real size (GPU)."""
import json
import os
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTSIDE_STEPS_S = 30.0   # a plain run: whole process, start to exit, less (steps + warmup) x ms_per_step
FULL_RUN_S = 600.0       # a --full run: whole process


def _run(extra, timeout_s):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "FENRIS_BENCH_CHILD"):
        env.pop(k, None)
    t0 = time.perf_counter()
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"] + extra,
                        env=env, cwd=ROOT, capture_output=True, text=True, timeout=timeout_s)
    seconds = time.perf_counter() - t0
    assert pr.returncode == 0, pr.stderr[-3000:]
    lines = [ln for ln in pr.stdout.splitlines() if ln.startswith("{") and '"metric"' in ln]
    assert len(lines) == 1, pr.stdout[-2000:]
    return json.loads(lines[0]), seconds


def _check_headline(line):
    assert line["metric"] == "elements/sec assembling global stiffness K, 3D Hex8 elasticity"
    assert line["unit"] == "elements/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    elements = 216 ** 3
    assert abs(line["value"] * line["ms_per_step"] * 1e-3 - elements) <= 1e-6 * elements
    assert line["roofline"]["kernel"] == "k_affine_rows" and 0.0 < line["roofline"]["frac"] < 1.0


def test_full_is_an_option_and_off_by_default():
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert pr.returncode == 0 and "--full" in pr.stdout
    # (the parser takes it: what is refused here is --steps 0, as without it)
    pr = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert pr.returncode == 2 and "--steps" in pr.stderr and "unrecognized" not in pr.stderr


@pytest.mark.gpu
def test_plain_run_is_the_headline_alone_and_short():
    line, seconds = _run([], 600)
    _check_headline(line)
    assert "secondary" not in line and "secondary_vectors" not in line
    assert line["cpu_baseline"] is None
    roof = line["roofline"]
    assert roof["traffic"] is None and "traffic_detail" not in roof and "measured_write_GBps" not in roof
    # the set-up of the timed steps is the same as under --full
    assert line["config"]["device_settle"] is not None and line["config"]["placement_probe"]["tries"] >= 1
    outside = seconds - (line["steps"] + line["warmup"]) * line["ms_per_step"] * 1e-3
    print(f"plain run: {seconds:.2f} s, {outside:.2f} s outside its steps")
    assert outside <= OUTSIDE_STEPS_S


@pytest.mark.gpu
def test_full_run_carries_everything_else():
    line, seconds = _run(["--full"], FULL_RUN_S)
    print(f"--full run: {seconds:.2f} s")
    assert seconds <= FULL_RUN_S
    _check_headline(line)
    assert sorted(line["secondary"]) == ["c2", "c3", "c4", "c5", "ns-perturbed"]
    for name, sec in line["secondary"].items():
        assert "error" not in sec and sec["ms"] > 0 and 0.0 < sec["frac"] < 1.0, (name, sec)
    sv = line["secondary_vectors"]
    assert "error" not in sv and sv["residual_ms"] > 0 and sv["energy_ms_blocking_call"] > 0
    assert line["cpu_baseline"]["value"] > 0 and line["cpu_baseline"]["unit"] == "elements/s"
    roof = line["roofline"]
    assert roof["measured_write_GBps"] > 0
    assert "traffic_detail" in roof   # (the passes ran; a profiler that could not count says so there and leaves traffic null)
    if "error" not in roof["traffic_detail"]:
        # every value is written once: 8 nnz bytes of the 12 nnz + ... algorithmic ones (0.65 of them on this mesh)
        assert roof["traffic"] >= 8 * line["config"]["nnz_per_gpu"]
