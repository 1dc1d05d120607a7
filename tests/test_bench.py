"""bench.py as its callers use it: a plain run prints the headline line only, --steps sets the timed steps,
--dump-outputs writes what the timed run computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_small_arrays_are_written_whole(tmp_path):
    x = np.linspace(-1.0, 1.0, 1000)
    order = np.arange(1000, dtype=np.uint64)[::-1]
    bench.dump_outputs(str(tmp_path), {"positions": x, "order": order})
    a, b = np.load(tmp_path / "positions.npy"), np.load(tmp_path / "order.npy")
    assert a.dtype == np.float64 and np.array_equal(a, x)
    assert b.dtype == np.float64 and np.array_equal(b, order.astype(np.float64))


def test_dump_outputs_over_budget_keeps_one_fixed_sample(tmp_path):
    x = np.arange(10_000, dtype=np.float64)
    y = -x
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"x": x, "y": y}, budget=16_000)
    xa, ya, xb = (np.load(tmp_path / d / f) for d, f in (("a", "x.npy"), ("a", "y.npy"), ("b", "x.npy")))
    assert xa.nbytes + ya.nbytes <= 16_000 and xa.size == 1000
    assert np.array_equal(xa, xb)                                  # seeded: the same entries every run
    assert np.array_equal(ya, -xa)                                 # the same entries of every array
    assert np.all(np.diff(xa) > 0)                                 # in index order


def test_bench_rejects_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "--steps" in r.stderr


@pytest.mark.gpu
def test_plain_bench_run_times_its_steps_and_dumps_outputs(tmp_path):
    steps, warmup = 3, 1
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup), "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["unit"] == "term-updates/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["steps"] == steps and out["warmup"] == warmup
    assert out["total_term_updates"] == steps * out["config"]["term_updates_per_step"]
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert out["value"] == pytest.approx(out["total_term_updates"] / (steps * out["ms_per_step"] * 1e-3))
    for extra in ("quality", "bubbles", "reference_streams", "layout_2d", "cpu_baseline", "wall_clock_pY"):
        assert extra not in out                                    # --full only
    x, order = np.load(tmp_path / "positions.npy"), np.load(tmp_path / "order.npy")
    assert x.dtype == np.float64 and order.dtype == np.float64
    assert x.shape == order.shape == (1_000_000,) and np.isfinite(x).all()
    o = order.astype(np.int64)
    assert np.array_equal(np.sort(o), np.arange(x.size)) and np.all(np.diff(x[o]) >= 0)
