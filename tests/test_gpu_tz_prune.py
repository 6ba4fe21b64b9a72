"""GPU parity of the raster pruning (tz_raster_cols_kernel: grid points that a block-sum lower bound rules out are not scanned): uniform all-uni rows through
vtmhip_xMotionEstimation_batch_dev -- the entry the benchmark's levels use -- against the oracle's xMotionEstimation, record by record and bit-exact, with the box sums
attached, with nothing attached, and (a child process) with VTMHIP_TZ_PRUNE=0.  The statistic of the context (vtmhip_tz_prune_stats) says what the bound did: the last test
requires skipped, reduced and accepted scans over the file's job sets, the controls require that jobs the bound does not apply to are left alone."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import me_util
from test_gpu_mest import hip_jobs
from test_gpu_tz_bands import CFGV, band_jobs
from vtm_amd.lib import MeCfg, MeOut, PicParams

PRUNE_OFF = os.environ.get("VTMHIP_TZ_PRUNE") == "0"      # (the child of test_prune_switched_off)
COPIES = 7      # 100 rows: rasterParts 8 (several workgroups share a scan); 700 rows (> 640): one workgroup per scan


def scene_of(kind):
    if kind == "hard":
        return me_util.Scene(832, 480, hard=True)
    if kind in ("easy", "easy_true", "easy_off8"):
        return me_util.Scene(832, 480, hard=False, t_cur=4)      # (a pan of (12, 8): at (6, 4) the diamond reaches the motion and no search comes to a scan)
    return me_util.DeepScene(832, 480, hard=True, bit_depth={"hard8": 8, "hard12": 12}[kind])


def jobs_of(kind, w, h):
    """band_jobs on the scene: search ranges 64 / 96 through the column kernel, 192 in-kernel, border PUs with one-sided windows, predictors far from the motion.
    easy_true: the same rows on the pure pan (t_cur - t_ref = 4: motion (12, 8)) with the predictor at the true motion.  easy_off8: with the predictor eight samples beside
    it -- the diamond lands on the motion itself at distance 8, the search comes to the scan holding the minimum, and the bound rules the whole grid out."""
    scene, jobs = band_jobs(w, h, 100, scene_of(kind))
    if kind == "easy_true":
        for j in jobs:
            j["cands"] = [[12 * 16, 8 * 16], [12 * 16, 8 * 16]]
            j["mvPred"] = (12 * 16, 8 * 16)
    if kind == "easy_off8":
        for j in jobs:
            j["cands"] = [[20 * 16, 8 * 16], [20 * 16, 8 * 16]]
            j["mvPred"] = (20 * 16, 8 * 16)
    if kind in ("hard8", "hard12"):
        lams = me_util.real_lambdas(scene.bd)
        for k, j in enumerate(jobs):
            j["lam"] = lams[(k // 7) % 5]
    return scene, jobs


def run_device(ctx, scene, jobs, w, h, wpj, attach, copies=1):
    """the rows (copies times over) through vtmhip_xMotionEstimation_batch_dev; attach: the box sums of the scene's reference plane are computed and attached for the call.
    Returns (records, integer results, the context's pruning statistic of this call)."""
    others = np.zeros(1, np.int16)
    arr = hip_jobs(scene, jobs, others)
    raw = np.tile(np.frombuffer(arr, np.uint8), copies)
    n = len(jobs) * copies
    cfg = MeCfg(CFGV[0], CFGV[1], CFGV[2], CFGV[3], CFGV[4], 0, 1, 1, 0, 0)      # uniformImv 0, uniformSquare, uniformBi 1 (all uni)
    pic = PicParams(scene.W, scene.H, 128, getattr(scene, "bd", 10), wpj)
    d_cur, d_ref, d_oth = ctx.to_device(scene.cur), ctx.to_device(scene.ref_buf), ctx.to_device(others)
    d_jobs, d_res = ctx.to_device(raw), ctx.alloc(C.sizeof(MeOut) * n)
    d_sums = None
    if attach:
        d_sums = ctx.alloc(2 * scene.ref_buf.size)
        ctx.tz_box_sums(d_ref.ptr, d_sums.ptr, scene.ref_off, scene.ref_stride, scene.W, scene.H, scene.margin)
        ctx.tz_attach_sums(d_ref.ptr, d_sums.ptr, scene.W, scene.H, scene.margin)
    ctx.tz_prune_stats(reset=True)
    try:
        ctx.motion_estimation_batch(pic, cfg, d_cur.ptr, d_ref.ptr, d_oth.ptr, d_jobs.ptr, n, w, h, d_res.ptr)
        stats = ctx.tz_prune_stats()
    finally:
        ctx.tz_attach_sums(None, None)
    res = (MeOut * n).from_buffer_copy(d_res.to_host(np.uint8).tobytes())
    for d in (d_cur, d_ref, d_oth, d_jobs, d_res, d_sums):
        if d is not None:
            d.free()
    return [(r.mvHor, r.mvVer, r.mvPredHor, r.mvPredVer, r.mvpIdx, r.bits, r.cost) for r in res], [(r.intX, r.intY, r.intDist) for r in res], stats


_CASES = {}


def case(ctx, kind, w, h, wpj, copies=1):
    """One job set against the oracle, with and without the sums; computed once per session (the oracle's records once per job set).  Returns the statistic of the attached
    run."""
    key = (kind, w, h, wpj, copies)
    if key in _CASES:
        return _CASES[key]
    okey = ("oracle", kind, w, h)
    if okey not in _CASES:
        scene, jobs = jobs_of(kind, w, h)
        _CASES[okey] = (scene, jobs) + me_util.run_oracle_mest(scene, jobs, CFGV)
    scene, jobs, exp, exp_int = _CASES[okey]
    exp, exp_int = exp * copies, exp_int * copies
    got, got_int, stats = run_device(ctx, scene, jobs, w, h, wpj, True, copies)
    bad = [k for k in range(len(exp)) if got[k] != exp[k] or got_int[k] != exp_int[k]]
    assert not bad, ("sums attached", stats, bad[:10], [(got[k], exp[k], got_int[k], exp_int[k], jobs[k % len(jobs)]["searchRange"]) for k in bad[:3]])
    got0, got_int0, stats0 = run_device(ctx, scene, jobs, w, h, wpj, False, copies)
    assert got0 == exp and got_int0 == exp_int, ("nothing attached", stats0)
    print("prune case", key, stats, "unattached", stats0)
    # nothing attached (or switched off): every listed scan runs whole
    assert stats0["skipped"] == 0 and stats0["reduced"] == 0 and stats0["points_evaluated"] == stats0["points_total"] and stats0["listed"] == stats["listed"], (stats, stats0)
    assert stats0["accepted"] == stats["accepted"] and stats0["points_total"] == stats["points_total"], (stats, stats0)
    if PRUNE_OFF:
        assert stats == stats0, (stats, stats0)
    _CASES[key] = stats
    return stats


SETS = [("hard", 128, 128, 8, 1), ("hard", 128, 64, 8, 1), ("hard", 128, 128, 8, COPIES), ("easy", 128, 128, 8, 1), ("easy", 128, 64, 8, 1), ("easy", 128, 128, 8, COPIES),
        ("easy_true", 128, 128, 8, 1), ("easy_true", 128, 64, 8, 1), ("easy_off8", 128, 128, 8, 1), ("easy_off8", 128, 64, 8, 1), ("hard8", 128, 128, 8, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,w,h,wpj,copies", SETS)
def test_pruned_scan_matches_oracle(ctx, kind, w, h, wpj, copies):
    st = case(ctx, kind, w, h, wpj, copies)
    assert st["listed"] > 0 or kind == "easy_true", st      # (with the predictor at the true motion few searches reach a scan at all)


@pytest.mark.gpu
def test_12bit_takes_the_unpruned_path(ctx):
    """64 * 4095 does not fit the 16-bit sums: with sums attached every scan runs whole, and the records match"""
    st = case(ctx, "hard12", 128, 128, 8)
    assert st["listed"] > 0 and st["skipped"] == 0 and st["reduced"] == 0 and st["points_evaluated"] == st["points_total"], st


@pytest.mark.gpu
def test_row_subsampled_shape_is_not_pruned(ctx):
    """64x64 (subShift 1: the SAD visits every other row, the 8x8 sums do not bound it) with sums attached"""
    st = case(ctx, "hard", 64, 64, 4)
    assert st["listed"] > 0 and st["skipped"] == 0 and st["reduced"] == 0 and st["points_evaluated"] == st["points_total"], st


@pytest.mark.gpu
def test_box_sums_against_numpy(ctx):
    """vtmhip_tz_box_sums_dev alone: a 64x48 plane with margin 144 and an odd stride padding, every covered position -- the first and the last covered row and column
    among them -- against a numpy box sum; nothing outside the covered positions is written."""
    W, H, m = 64, 48, 144
    stride, rows = W + 2 * m + 5, H + 2 * m
    rng = np.random.default_rng(77)
    ext = rng.integers(0, 1024, (rows, stride)).astype(np.int16)
    cs = np.zeros((rows + 1, stride + 1), np.int64)
    cs[1:, 1:] = ext.astype(np.int64).cumsum(0).cumsum(1)
    box = cs[8:, 8:] - cs[:-8, 8:] - cs[8:, :-8] + cs[:-8, :-8]      # box[y, x] = sum of ext[y : y + 8, x : x + 8]
    exp = np.full((rows, stride), 0xffff, np.uint16)
    x0, x1, y0, y1 = m - (m - 9), m + W + m - 17, m - (m - 9), m + H + m - 17      # plane positions -(m - 9) .. size + m - 17 in buffer coordinates
    assert (x0, y0) == (9, 9) and x1 + 7 < W + 2 * m and y1 + 7 < rows
    exp[y0:y1 + 1, x0:x1 + 1] = box[y0:y1 + 1, x0:x1 + 1]
    d_ref, d_sums = ctx.to_device(ext.reshape(-1)), ctx.to_device(np.full(rows * stride, 0xffff, np.uint16))
    ctx.tz_box_sums(d_ref.ptr, d_sums.ptr, m * stride + m, stride, W, H, m)
    ctx.sync()
    got = d_sums.to_host(np.uint16).reshape(rows, stride)
    d_ref.free()
    d_sums.free()
    assert int(box[y0:y1 + 1, x0:x1 + 1].max()) < 0xffff
    for name, sl in (("first row", np.s_[y0, x0:x1 + 1]), ("last row", np.s_[y1, x0:x1 + 1]), ("first column", np.s_[y0:y1 + 1, x0]), ("last column", np.s_[y0:y1 + 1, x1])):
        assert np.array_equal(got[sl], exp[sl]), name
    assert np.array_equal(got, exp), np.argwhere(got != exp)[:10]


@pytest.mark.gpu
def test_pruning_is_not_vacuous(ctx):
    """Over the file's job sets the bound skips scans, reduces scans to a proper sub-rectangle, and leaves scans whose winner the search accepts"""
    tot = {}
    for s in SETS:
        for k, v in case(ctx, *s).items():
            tot[k] = tot.get(k, 0) + v
    print("prune totals", tot)
    if PRUNE_OFF:      # (the whole file under VTMHIP_TZ_PRUNE=0: nothing is pruned)
        assert tot["skipped"] == 0 and tot["reduced"] == 0 and tot["accepted"] >= 5, tot
        return
    assert tot["skipped"] >= 5 and tot["reduced"] >= 5 and tot["accepted"] >= 5, tot
    assert tot["points_evaluated"] < tot["points_total"], tot


@pytest.mark.gpu
def test_prune_switched_off():
    """VTMHIP_TZ_PRUNE=0 (read once per process: a child process): every job set of the file with sums attached -- every scan whole (case() compares the two
    statistics), the same records -- and the totals over the sets (nothing skipped, nothing reduced)."""
    if os.environ.get("VTMHIP_TEST_CHILD"):
        pytest.skip("the child itself")
    env = dict(os.environ, VTMHIP_TEST_CHILD="1", VTMHIP_TZ_PRUNE="0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k", "matches_oracle or not_vacuous"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "%d passed" % (len(SETS) + 1) in out, out[-3000:]
