"""bench.py --dump-outputs: the writer keeps to its size budget, draws the same row sample every time, and the argument checks run before any GPU work."""
import glob
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _tables():
    rng = np.random.default_rng(7)
    return {"L0_128x128_pus": rng.integers(0, 1 << 40, (510, 22), dtype=np.int64), "L4_8x8_pus": rng.integers(-512, 512, (130560, 22)),
            "L4_8x8_mts_test": rng.integers(0, 2, 783360).astype(np.uint8), "L4_8x8_tu_res": rng.integers(0, 1 << 30, (783360, 2), dtype=np.int64)}


def test_dump_keeps_budget_and_samples_the_same_rows(tmp_path):
    budget = 8 << 20
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    ia, ib = bench.dump_outputs(_tables(), a, budget), bench.dump_outputs(_tables(), b, budget)
    assert ia == dict(ib, dir=a)
    files = sorted(glob.glob(os.path.join(a, "*.npy")))
    payload = sum(np.load(f).nbytes for f in files)
    assert payload == ia["bytes"] <= budget
    assert "L4_8x8_pus" in ia["sampled"] and "L0_128x128_pus" not in ia["sampled"]
    for f in files:
        x, y = np.load(f), np.load(f.replace(a, b))
        assert x.dtype == np.float64 and x.ndim == (1 if f.endswith("_rows.npy") else 2) and np.array_equal(x, y), f
    # a sampled table holds exactly the rows its _rows file names
    rows = np.load(os.path.join(a, "L4_8x8_pus_rows.npy")).astype(np.int64)
    assert np.array_equal(np.load(os.path.join(a, "L4_8x8_pus.npy")), _tables()["L4_8x8_pus"][rows].astype(np.float64))
    # an unsampled table is written whole, values unchanged
    assert np.array_equal(np.load(os.path.join(a, "L0_128x128_pus.npy")), _tables()["L0_128x128_pus"].astype(np.float64))


def test_dump_removes_a_stale_row_list(tmp_path):
    d = str(tmp_path)
    bench.dump_outputs({"t": np.arange(4096.0).reshape(-1, 1)}, d, budget=4096)
    assert os.path.exists(os.path.join(d, "t_rows.npy"))
    bench.dump_outputs({"t": np.arange(16.0).reshape(-1, 1)}, d, budget=4096)
    assert not os.path.exists(os.path.join(d, "t_rows.npy"))


def test_dump_and_steps_arguments_are_checked_before_gpu_work():
    for args in (["--steps", "0"], ["--gpus", "2", "--dump-outputs", "x"]):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + ["--launch-check"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 2 and b"error" in p.stderr, (args, p.stderr[-500:])
