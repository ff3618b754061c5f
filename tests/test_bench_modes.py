"""bench.py's two modes.  A plain run carries the headline figure and nothing that takes a run or a check of its own;
`--full` adds those.  Both step the headline engine alike: the same arrays from `--dump-outputs`."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")

HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY_KEYS = ("roofline", "roofline_dominant", "cpu_baseline", "cpu_baseline_same_algorithm", "kernels_us")
# a small LP on the two-launch pipeline of the headline workload (m >= 384); 10 + 30 + 15 steps stay inside phase 1
SIZE = ["--m", "420", "--n", "1000", "--steps", "30", "--warmup", "10", "--long-window", "15"]


def test_full_is_an_option_that_is_off_by_default(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.full is False and (a.steps, a.warmup) == (7, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    assert bench.parse().full is True


def _run(extra, dump):
    cmd = [sys.executable, BENCH, "--gpus", "1"] + SIZE + ["--dump-outputs", str(dump)] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(dump, f)) for f in sorted(os.listdir(dump))}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bench_modes")
    return {"plain": _run([], d / "plain"),
            "full": _run(["--full", "--cpu-pivots", "3", "--same-alg-pivots", "40", "--profile-steps", "20"], d / "full")}


@pytest.mark.gpu
def test_plain_line_has_the_headline_and_nothing_measured_apart(runs):
    line, _ = runs["plain"]
    for k in HEADLINE_KEYS:
        assert k in line, k
    assert line["full"] is False and line["unit"] == "pivots/s" and line["dtype"] == "f64" and line["higher_is_better"] is True
    assert line["steps"] == 30 and line["value"] > 0 and line["ms_per_step"] == pytest.approx(1e3 / line["value"], rel=1e-4)
    for k in FULL_ONLY_KEYS:
        assert k not in line, k
    assert "inverse_residual_after" not in line["config"]


@pytest.mark.gpu
def test_full_line_has_what_moved(runs):
    line, _ = runs["full"]
    for k in HEADLINE_KEYS + FULL_ONLY_KEYS:
        assert k in line, k
    assert line["full"] is True
    assert line["kernels_us"] and line["cpu_baseline"]["value"] > 0
    assert np.isfinite(line["config"]["inverse_residual_after"])
    assert line["long_window"]["steps"] == 15


@pytest.mark.gpu
def test_both_modes_dump_the_same_point(runs):
    (_, plain), (_, full) = runs["plain"], runs["full"]
    assert sorted(plain) == sorted(full) == ["basis", "nonbasic", "nonbasic_at", "objective", "status_iterations", "x"]
    assert plain["status_iterations"][1] == 10 + 30 + 15
    for name in plain:
        np.testing.assert_array_equal(plain[name], full[name], err_msg=name)
