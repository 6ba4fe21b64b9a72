"""GPU parity: integer motion search (one wave = one InterSearch::xTZSearch) vs the CPU oracle.  Bit-exact MV, cost,
distortion and evaluation count."""
import functools

import numpy as np
import pytest

import me_util
from vtm_amd.lib import MeResult, PicParams

pytestmark = pytest.mark.gpu


def _run_hip(ctx, scene, jobs, wpj=0, max_sr=0):
    arr = me_util.hip_tz_jobs(scene, jobs, scene.W)
    d_cur, d_ref = ctx.to_device(scene.cur), ctx.to_device(scene.ref_buf)
    d_jobs = ctx.to_device(np.frombuffer(arr, np.uint8))
    d_res = ctx.alloc(len(jobs) * 32)
    pic = PicParams(scene.W, scene.H, 128, getattr(scene, "bd", 10), wpj, max_sr)
    ctx.tz_search_batch(pic, d_cur.ptr, d_ref.ptr, d_jobs.ptr, len(jobs), d_res.ptr)
    raw = d_res.to_host(np.uint8)
    res = (MeResult * len(jobs)).from_buffer_copy(raw.tobytes())
    return [(r.mvX, r.mvY, r.cost, r.dist, r.nEval) for r in res]


@pytest.mark.parametrize("hard", [True, False])
def test_tz_search_matches_oracle(ctx, hard):
    scene = me_util.Scene(416, 240, hard=hard)
    jobs = me_util.random_tz_jobs(scene, 1500, seed=5 if hard else 6)
    exp = me_util.run_oracle_tz(scene, jobs)
    got = _run_hip(ctx, scene, jobs)
    bad = [k for k in range(len(jobs)) if got[k] != exp[k]]
    assert not bad, [(jobs[k], got[k], exp[k]) for k in bad[:5]]


def test_tz_search_picture_border_and_tiny_range(ctx):
    """PUs on the picture border with large predictors (clipMv / xClipMv active) and searchRange 1..4."""
    scene = me_util.Scene(416, 240, hard=True)
    jobs = me_util.random_tz_jobs(scene, 400, seed=9, ranges=(1, 2, 4, 384))
    for k, j in enumerate(jobs):
        if k % 2 == 0:
            j["x"] = 0 if k % 4 == 0 else scene.W - j["w"]
            j["y"] = 0 if k % 8 < 4 else scene.H - j["h"]
            j["mvHor"], j["mvVer"] = (-1) ** k * 3000, (-1) ** (k // 2) * 2500
    exp = me_util.run_oracle_tz(scene, jobs)
    got = _run_hip(ctx, scene, jobs)
    bad = [k for k in range(len(jobs)) if got[k] != exp[k]]
    assert not bad, [(jobs[k], got[k], exp[k]) for k in bad[:5]]


def test_tz_search_signed_samples(ctx):
    """Full int16 range targets (2*org - pred of bi-pred ME) through the sign-biased v_sad_u16 path."""
    scene = me_util.Scene(416, 240, hard=True)
    rng = np.random.default_rng(17)
    scene.cur = np.ascontiguousarray((2 * scene.cur.astype(np.int32) - rng.integers(0, 1024, scene.cur.shape)).astype(np.int16))
    assert scene.cur.min() < 0
    jobs = me_util.random_tz_jobs(scene, 500, seed=18)
    for j in jobs:
        j["signed"] = 1
    exp = me_util.run_oracle_tz(scene, jobs)
    got = _run_hip(ctx, scene, jobs)
    bad = [k for k in range(len(jobs)) if got[k] != exp[k]]
    assert not bad, [(jobs[k], got[k], exp[k]) for k in bad[:5]]


@pytest.mark.parametrize("wpj", [2, 4, 8, 16])
def test_tz_search_multi_wave_jobs(ctx, wpj):
    """wavesPerJob > 1: the waves of a workgroup split every candidate list; results must not change."""
    scene = me_util.Scene(416, 240, hard=True)
    jobs = me_util.random_tz_jobs(scene, 400, seed=30 + wpj)
    exp = me_util.run_oracle_tz(scene, jobs)
    got = _run_hip(ctx, scene, jobs, wpj)
    bad = [k for k in range(len(jobs)) if got[k] != exp[k]]
    assert not bad, [(jobs[k], got[k], exp[k]) for k in bad[:5]]


@pytest.mark.parametrize("wpj,max_sr", [(0, 384), (8, 384), (2, 192), (0, 130)])
def test_tz_search_large_search_ranges_through_the_column_scan(ctx, wpj, max_sr):
    """vtmhip_pic_params::maxSearchRange sizes the raster column kernel's LDS totals for ASR ranges up to 384 (154 x 154 scan points): the scans of SearchRange 192 / 384 jobs then
    run in tz_raster_cols_kernel instead of inside the search kernel -- same results (scans larger than the hint still take the in-kernel path)."""
    scene = me_util.Scene(832, 480, hard=True)
    jobs = me_util.random_tz_jobs(scene, 300, seed=70 + wpj, ranges=(96, 192, 384))
    for k, j in enumerate(jobs):      # far-off predictors: the first search ends >= 5 samples from its start, so the raster scan runs
        j["mvHor"], j["mvVer"] = (-1) ** k * (400 + 16 * (k % 40)), (-1) ** (k // 2) * (300 + 16 * (k % 23))
    exp = me_util.run_oracle_tz(scene, jobs)
    got = _run_hip(ctx, scene, jobs, wpj, max_sr)
    bad = [k for k in range(len(jobs)) if got[k] != exp[k]]
    assert not bad, [(jobs[k], got[k], exp[k]) for k in bad[:5]]
    assert sum(1 for e in exp if e[4] > 2000) >= 50      # many searches really scanned a large window (nEval counts the scan points)


# ---- 8 / 12-bit pictures, the reference's lambdas up to QP 63, and the limits of the arg-min keys ----------------------------------------------------------------
def _check_keys(ctx, scene, jobs, wpj, max_sr=0, floors=("tiny", "narrow", "wide"), exp=None):
    """Device = oracle, job by job; the jobs provably reach each arg-min key the test claims (MeJob::tiny / narrow / the 64-bit compare)."""
    for j in jobs:
        j["signed"] = getattr(scene, "signed", 0)
    exp = exp or me_util.run_oracle_tz(scene, jobs)
    cls = me_util.key_classes(jobs, scene.bd)
    assert all(cls[c] >= 20 for c in floors), cls
    got = _run_hip(ctx, scene, jobs, wpj, max_sr)
    bad = [k for k in range(len(jobs)) if got[k] != exp[k]]
    assert not bad, (len(bad), [(jobs[k], got[k], exp[k]) for k in bad[:5]])
    return exp


@pytest.mark.parametrize("wpj", [0, 2, 8])
@pytest.mark.parametrize("signed", [0, 1])
@pytest.mark.parametrize("bd", [8, 12])
def test_tz_search_8_12bit_real_and_edge_lambdas(ctx, bd, signed, wpj):
    """The integer search on 8- and 12-bit pictures (plain and 2*org - pred targets of the depth's range) with the motion lambdas of QP 22 .. 63 at that depth and three
    beyond every real one: 6e5 (no shape keeps the one-word key), 2e7 and 3e9 (lambda * 126 >= 2^31: the 64-bit arg-min)."""
    scene = me_util.DeepScene(416, 240, hard=True, bit_depth=bd)
    if signed:
        me_util.make_signed(scene, 40 + bd)
        assert scene.cur.min() < -(1 << (bd - 1)) and scene.cur.max() > (1 << bd)
    jobs = me_util.random_tz_jobs(scene, 400, seed=500 + 10 * bd + 3 * signed + wpj, lams=me_util.real_lambdas(bd) + me_util.EDGE)
    _check_keys(ctx, scene, jobs, wpj)


@functools.lru_cache(maxsize=None)
def _saturated_case(bd, signed):
    """Scene, jobs and the oracle's results (the same for every wavesPerJob: computed once): 200 jobs of every shape + 150 of 128x128 / 128x64 / 64x128 / 64x64, the second
    list under real lambdas only (its costs are distortion)"""
    scene = me_util.SaturatedScene(416, 240, bd, seed=60 + bd, signed=bool(signed))
    jobs = (me_util.random_tz_jobs(scene, 200, seed=600 + 10 * bd + 3 * signed, lams=me_util.real_lambdas(bd) + me_util.EDGE) +
            me_util.random_tz_jobs(scene, 150, seed=601 + 10 * bd + 3 * signed, sizes=me_util.BIG, lams=me_util.real_lambdas(bd)))
    return scene, jobs, me_util.run_oracle_tz(scene, jobs)


@pytest.mark.parametrize("wpj", [0, 2, 8])
@pytest.mark.parametrize("signed", [0, 1])
@pytest.mark.parametrize("bd", [8, 10, 12])
def test_tz_search_saturated_scene(ctx, bd, signed, wpj):
    """Block SADs of about w * h * (2^bd - 1): partial sums, the sample range and -- at 12 bits -- distortions at the limit of the one-word key (128x128: 67 092 480 of
    2^26 = 67 108 864) and, signed, beyond it."""
    scene, jobs, exp = _saturated_case(bd, signed)
    assert sum(1 for j in jobs if j["w"] * j["h"] >= 128 * 64) * 3 >= len(jobs)
    _check_keys(ctx, scene, jobs, wpj, exp=exp)
    if bd == 12:
        assert me_util.near_key_limit(jobs, [e[2] for e in exp], [e[3] for e in exp], bd, signed) >= 10


def test_tz_search_saturated_scene_through_the_column_scan(ctx):
    """The raster column kernel (maxSearchRange 384) on the 12-bit saturated scene: column totals of 128-wide blocks at w * h * max."""
    scene = me_util.SaturatedScene(832, 480, 12, seed=81)
    lams = me_util.real_lambdas(12) + me_util.EDGE
    jobs = (me_util.random_tz_jobs(scene, 150, seed=82, ranges=(96, 192, 384), lams=lams) +
            me_util.random_tz_jobs(scene, 150, seed=83, ranges=(96, 192, 384), sizes=me_util.BIG, lams=me_util.real_lambdas(12)))
    for k, j in enumerate(jobs):      # far-off predictors: the raster scan runs
        j["mvHor"], j["mvVer"] = (-1) ** k * (400 + 16 * (k % 40)), (-1) ** (k // 2) * (300 + 16 * (k % 23))
    exp = _check_keys(ctx, scene, jobs, 0, 384, floors=("tiny", "narrow"))
    assert sum(1 for e in exp if e[4] > 2000) >= 50
    assert me_util.near_key_limit(jobs, [e[2] for e in exp], [e[3] for e in exp], 12, 0) >= 10


@pytest.mark.parametrize("bd", [0, 7, 13, 16])
def test_bit_depth_out_of_range_returns_status(ctx, bd):
    """pic->bitDepth outside 8 .. 12 (the library's sample contract): the three search entries return an error and launch nothing (the result buffers keep their bytes)."""
    import ctypes as C
    from vtm_amd.lib import FullJob, MeCfg, MeOut, VtmHipError
    from test_gpu_mest import hip_jobs
    scene = me_util.Scene(416, 240, hard=True)
    pic = PicParams(scene.W, scene.H, 128, bd, 0, 0)
    d_cur, d_ref = ctx.to_device(scene.cur), ctx.to_device(scene.ref_buf)
    mark = np.full(4 * 64, 0x5a, np.uint8)
    # xTZSearch entry
    jobs = me_util.random_tz_jobs(scene, 4, seed=1)
    d_jobs, d_res = ctx.to_device(np.frombuffer(me_util.hip_tz_jobs(scene, jobs, scene.W), np.uint8)), ctx.to_device(mark)
    with pytest.raises(VtmHipError):
        ctx.tz_search_batch(pic, d_cur.ptr, d_ref.ptr, d_jobs.ptr, 4, d_res.ptr)
    assert np.array_equal(d_res.to_host(np.uint8), mark)
    # xPatternSearch entry: the cooperative kernel and the lane-per-candidate one
    fj = (FullJob * 4)()
    for k, j in enumerate(fj):
        j.orgOff, j.refOff = 16 * k, scene.ref_off + 16 * k
        j.orgStride, j.refStride, j.puX, j.puY, j.width, j.height = scene.W, scene.ref_stride, 16 * k, 0, 16, 16
        j.motionLambda, j.searchRange = 8.0, 4
    d_fj = ctx.to_device(np.frombuffer(fj, np.uint8))
    for square in (0, 16):
        with pytest.raises(VtmHipError):
            ctx.full_search_batch(pic, d_cur.ptr, d_ref.ptr, d_fj.ptr, 4, d_res.ptr, square=square)
        assert np.array_equal(d_res.to_host(np.uint8), mark)
    # xMotionEstimation entry: a small batch (one chain) and one large enough to be bucketed by shape
    for n in (4, 80):
        mj = me_util.random_mest_jobs(scene, n, seed=2)
        others = np.zeros(max(1, sum(j["w"] * j["h"] for j in mj if j["bi"])), np.int16)
        d_mj, d_oth = ctx.to_device(np.frombuffer(hip_jobs(scene, mj, others), np.uint8)), ctx.to_device(others)
        d_out = ctx.to_device(np.full(C.sizeof(MeOut) * n, 0x5a, np.uint8))
        with pytest.raises(VtmHipError):
            ctx.motion_estimation_batch(pic, MeCfg(4, 1, 1, 0, 1, -1, 0, 0, 0, 0), d_cur.ptr, d_ref.ptr, d_oth.ptr, d_mj.ptr, n, 128, 128, d_out.ptr)
        assert np.all(d_out.to_host(np.uint8) == 0x5a)
