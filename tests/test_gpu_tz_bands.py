"""GPU parity of the row-band form of tz_search_kernel (a thread keeps K segments of the block for the whole search, a round loads all its candidates at once): uniform
all-uni rows through vtmhip_xMotionEstimation_batch_dev -- the entry the benchmark's levels use -- against the oracle's xMotionEstimation, record by record and bit-exact.
vtmhip_tz_band_items decides which launches take the band kernels; the cases cover every (shape, wavesPerJob) instantiation it accepts plus two it rejects."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import me_util
import oracle_lib as ol
from test_gpu_mest import hip_jobs
from vtm_amd.lib import MeCfg, MeOut, PicParams

CFGV = (4, 1, 1, 0, 1)      # BipredSearchRange 4, HadamardME, FastInterSearchMode 1 / 3 (row sub-sampling), no extended settings, first-search stop

# (w, h, wavesPerJob) -> the band kernel runs
ACCEPTED = [(32, 32, 1), (64, 64, 2), (64, 64, 4), (128, 128, 8), (128, 128, 16), (128, 64, 8), (64, 128, 4), (64, 32, 2), (32, 64, 2), (64, 128, 2)]
REJECTED = [(64, 64, 8), (32, 32, 2)]      # the block does not cover 64 * wavesPerJob threads: today's kernel through the same entry


def sub_shift(cfgv, w, h):
    """mg::sub_shift of the launch's cfg (RdCost.cpp:289-323, mode 2)"""
    return 1 if cfgv[2] and h > 8 and w <= 64 else 0


def run_device(ctx, scene, jobs, cfgv, waves_per_job, max_wh):
    """test_gpu_mest.run_device for uniform all-uni rows, with pic.wavesPerJob as a parameter"""
    others = np.zeros(1, np.int16)
    arr = hip_jobs(scene, jobs, others)
    cfg = MeCfg(cfgv[0], cfgv[1], cfgv[2], cfgv[3], cfgv[4], 0, 1, 1, 0, 0)      # uniformImv 0, uniformSquare, uniformBi 1 (all uni)
    pic = PicParams(scene.W, scene.H, 128, getattr(scene, "bd", 10), waves_per_job)
    d_cur, d_ref, d_oth = ctx.to_device(scene.cur), ctx.to_device(scene.ref_buf), ctx.to_device(others)
    d_jobs = ctx.to_device(np.frombuffer(arr, np.uint8))
    d_res = ctx.alloc(C.sizeof(MeOut) * len(jobs))
    ctx.motion_estimation_batch(pic, cfg, d_cur.ptr, d_ref.ptr, d_oth.ptr, d_jobs.ptr, len(jobs), max_wh[0], max_wh[1], d_res.ptr)
    res = (MeOut * len(jobs)).from_buffer_copy(d_res.to_host(np.uint8).tobytes())
    return [(r.mvHor, r.mvVer, r.mvPredHor, r.mvPredVer, r.mvpIdx, r.bits, r.cost) for r in res], [(r.intX, r.intY, r.intDist) for r in res]


def band_jobs(w, h, n, scene=None):
    """The job mix of test_four_searches_per_wave_integer_kernel on a picture that holds 128x128 blocks: search ranges 1 .. 192 (empty loops, one-round loops, raster scans
    listed for the column kernel and resumed, and -- 192 -- scans too large for it that run inside the search kernel), 0 .. 15 m_uniMvList entries with duplicates, cached
    integer vectors (fast settings), predictors next to the zero vector and far from the true motion, PUs on the picture border."""
    scene = scene or me_util.Scene(832, 480, hard=True)
    jobs = me_util.random_mest_jobs(scene, n, seed=8100 + 64 * w + h, sizes=([w], [h]))
    rng = np.random.default_rng(11 + w + h)
    for k, j in enumerate(jobs):
        j["imv"], j["bi"] = 0, 0
        j["cands"] = [[me_util._round_amvr(v, 0) for v in c] for c in j["cands"]]
        j["mvPred"] = tuple(j["cands"][j["mvpIdx"]])
        j["searchRange"] = [1, 2, 4, 8, 64, 96, 192][k % 7]
        m = k % 16
        extra = [(int(rng.integers(-12 * 16, 12 * 16)), int(rng.integers(-12 * 16, 12 * 16))) for _ in range(m)]
        if m >= 3 and k % 2:
            extra[m - 1] = extra[0]                    # a duplicate at the end (with 15 entries: no second round)
        if m >= 4 and k % 3 == 0:
            extra[2] = extra[1]
        j["extra"] = extra
        j["cached"] = int(k % 5 == 0)
        if k % 4 == 0:                                 # a predictor next to the zero vector: the zero candidate wins or ties the start round
            j["cands"] = [[0, 0], [16, 0]]
            j["mvPred"] = tuple(j["cands"][j["mvpIdx"]])
        if k % 6 == 1:                                 # on the picture border: the clipped search window is one-sided
            j["x"] = 0 if k % 12 == 1 else scene.W - w
        if k % 6 == 4:
            j["y"] = 0 if k % 12 == 4 else scene.H - h
    return scene, jobs


def check_case(ctx, w, h, wpj, expect_band, scene=None):
    """scene: a picture at another depth -- its rows take the motion lambdas of QP 22 / 32 / 33 / 51 / 63 at that depth in turn (12-bit 128x128: 125.3 / 140.7 at QP 32 / 33,
    either side of the one-word key's limit 130.03)"""
    k_band = ctx.tz_band_items(w, h, sub_shift(CFGV, w, h), wpj)
    assert (k_band > 0) == expect_band, (w, h, wpj, k_band)
    deep = scene is not None
    scene, jobs = band_jobs(w, h, 100 if w * h >= 128 * 64 else 200, scene)
    if deep:
        lams = me_util.real_lambdas(scene.bd)
        for k, j in enumerate(jobs):
            j["lam"] = lams[(k // 7) % 5]      # (k % 7 is the search range: every range under every lambda)
        if (w, h, scene.bd) == (128, 128, 12):
            assert sum(1 for j in jobs if j["lam"] < 130.03) >= 10 and sum(1 for j in jobs if j["lam"] > 130.03) >= 10
            assert me_util.key_classes(jobs, 12)["tiny"] >= 10 and me_util.key_classes(jobs, 12)["narrow"] >= 10
    L = ol.oracle()
    cfg = ol.MestCfg(*CFGV)
    exp, exp_int = [], []
    for j in jobs:
        keep = []
        t = me_util.oracle_mest_job(scene, j, keep)
        r = ol.MestResult()
        L.vo_motion_estimation(C.byref(cfg), C.byref(t), C.byref(r))
        exp.append(r.key())
        exp_int.append((r.intX, r.intY, r.intDist))
    got, got_int = run_device(ctx, scene, jobs, CFGV, wpj, (w, h))
    bad = [k for k in range(len(jobs)) if got[k] != exp[k] or got_int[k] != exp_int[k]]
    assert not bad, (k_band, bad[:10], [(got[k], exp[k], got_int[k], exp_int[k], jobs[k]["searchRange"], len(jobs[k]["extra"]), jobs[k]["cached"]) for k in bad[:3]])


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,wpj", ACCEPTED)
def test_band_kernel_matches_oracle(ctx, w, h, wpj):
    check_case(ctx, w, h, wpj, True)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,wpj", ACCEPTED)
def test_band_kernel_matches_oracle_12bit(ctx, w, h, wpj):
    check_case(ctx, w, h, wpj, True, me_util.DeepScene(832, 480, hard=True, bit_depth=12))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,wpj", [(32, 32, 1), (64, 64, 2), (128, 128, 8), (128, 64, 8)])
def test_band_kernel_matches_oracle_8bit(ctx, w, h, wpj):
    check_case(ctx, w, h, wpj, True, me_util.DeepScene(832, 480, hard=True, bit_depth=8))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,wpj", [(128, 128, 8), (128, 128, 16), (128, 64, 8), (64, 64, 4)])
def test_band_kernel_saturated_scene_12bit(ctx, w, h, wpj):
    """Distortions of about w * h * 4095: at 128x128 the rows under QP 22 / 32 keep the one-word key with costs within a factor of two of its limit"""
    scene = me_util.SaturatedScene(832, 480, 12, seed=91)
    check_case(ctx, w, h, wpj, True, scene)
    if (w, h) == (128, 128):
        _, jobs = band_jobs(w, h, 100, scene)
        lams = me_util.real_lambdas(12)
        for k, j in enumerate(jobs):
            j["lam"] = lams[(k // 7) % 5]
        exp, exp_int = me_util.run_oracle_mest(scene, jobs, CFGV)
        # (the integer search's distortion stands in for its cost: cost >= dist, and a "tiny" job's cost is < 2^26 whatever the candidate)
        assert me_util.near_key_limit(jobs, [e[2] for e in exp_int], [e[2] for e in exp_int], 12, 0) >= 10


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,wpj", REJECTED)
def test_rejected_shapes_keep_the_candidate_kernel(ctx, w, h, wpj):
    check_case(ctx, w, h, wpj, False)


def test_band_predicate():
    """vtmhip_tz_band_items on the host alone: K = segments / (64 * wavesPerJob) when that is 1, 2 or 4 and the shape has 8-sample segments and a power-of-two row length."""
    from vtm_amd import lib
    f = lib.load().vtmhip_tz_band_items
    assert [f(128, 128, 0, 8), f(128, 128, 0, 16), f(128, 128, 0, 4), f(64, 64, 1, 2), f(64, 64, 1, 4), f(32, 32, 1, 1), f(32, 32, 1, 0)] == [4, 2, 0, 2, 1, 1, 1]
    assert [f(64, 32, 1, 2), f(32, 64, 1, 2), f(128, 64, 0, 8), f(64, 128, 1, 4)] == [1, 1, 2, 2]
    for w, h, ss, wpj in [(48, 48, 1, 1), (24, 32, 1, 1), (12, 16, 1, 1), (4, 8, 0, 1), (64, 64, 1, 8), (32, 32, 1, 2), (16, 16, 1, 1), (64, 64, 1, 3), (64, 64, 0, 1), (128, 128, 0, 2)]:
        assert f(w, h, ss, wpj) == 0, (w, h, ss, wpj)


def _child(env_extra):
    if os.environ.get("VTMHIP_TEST_CHILD"):
        pytest.skip("the child itself")
    env = dict(os.environ, VTMHIP_TEST_CHILD="1", **env_extra)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k", "matches_oracle and not 8bit and ((32-32-1 or 64-64-2) and not 12bit or 128-128-8)"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "4 passed" in out, out[-3000:]


@pytest.mark.gpu
def test_bands_switched_off():
    """VTMHIP_TZ_BANDS=0 (read once per process: a child process): the same launches through the by-candidate kernel, the same results."""
    _child({"VTMHIP_TZ_BANDS": "0"})


@pytest.mark.gpu
def test_band_kernels_with_in_kernel_raster_scans():
    """VTMHIP_TZ_SPLIT=0: every raster scan runs inside the band kernels (the original block is staged in LDS when a scan is reached)."""
    _child({"VTMHIP_TZ_SPLIT": "0"})
