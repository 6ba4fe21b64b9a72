"""bench.py: a plain run measures only the headline (value, ms_per_step); the side figures that take runs of their own -- per-stage and per-kernel
times, the SATD micro-benchmark, the rooflines, the PCIe upload, the CPU baselines -- come with --full.  A small picture keeps both runs short."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE_KEYS = {"stages_ms", "kernels", "satd_gblocks_per_s", "integer_search", "roofline", "satd_roofline", "satd_grid_sizes", "pcie", "cpu_baseline"}


def _line(args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--width", "256", "--height", "128", "--steps", "2", "--warmup", "1"] + args,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_headline_only_and_full_adds_the_side_figures():
    plain = _line([])
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["unit"] == "pictures/s" and plain["higher_is_better"] is True
    assert not SIDE_KEYS & set(plain), sorted(SIDE_KEYS & set(plain))
    full = _line(["--full", "--no-cpu-baseline"])
    assert {k: plain[k] for k in ("metric", "unit", "dtype", "higher_is_better")} == {k: full[k] for k in ("metric", "unit", "dtype", "higher_is_better")}
    assert {"stages_ms", "kernels", "satd_gblocks_per_s", "integer_search", "roofline", "satd_roofline", "pcie"} <= set(full), sorted(full)
    assert full["kernels"] and full["stages_ms"] and "cpu_baseline" not in full
