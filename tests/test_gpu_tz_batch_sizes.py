"""GPU parity of the integer search at the batch sizes where its host launcher (vtmhip_internal_tz_search, me.hip) changes the launch plan -- the sizes a level of a
3840x2160 picture has and no other test of the suite reaches:

  A  more listed raster scans than tz_raster_cols_kernel has workgroups (its loop over the list runs more than once in a workgroup and re-uses the LDS totals, the
     pruning rectangle and the reduction slots), and more listed searches than the bounded resume grid of tz_search_kernel<1> takes in one pass;
  B  every number of workgroups per scan (rasterParts 8 .. 1, with 1 .. 3 scans in the call among them);
  C  the large-scan hint (maxSearchRange 384) either side of the 64 MB bound of the global totals;
  D  vtmhip_bdof_batch_dev past the 65 535 PUs of one launch, and the DMVR entries' refusal of such a call.

Expected values come from the oracle alone (vo_tz_search, vo_motion_estimation, vo_bdof_pu), job by job and bit-exact; the plan a case is about is asserted from the
context's statistic (vtmhip_tz_prune_stats: `listed` = the scans the column kernel took), never assumed."""
import ctypes as C
import functools

import numpy as np
import pytest

import me_util
import oracle_lib as ol
from test_gpu_me import _run_hip
from test_gpu_mest import hip_jobs
from test_gpu_tz_bands import CFGV, band_jobs
from vtm_amd.lib import E_INVALID, DmvrJob, MeCfg, MeOut, PicParams, PredJob, VtmHipError

pytestmark = pytest.mark.gpu

# vtmhip_internal_tz_search (me.hip; the lines carry a comment that names this file):
COLS_GRID = 3072                  # the grid of tz_raster_cols_kernel when one workgroup takes a scan ("n < 3072 ? n : 3072" at its launch): with more listed scans its loop
#                                   "for( e = ...; e < count; e += eStride )" runs more than once in a workgroup
RESUME_GRID = 2048                # the cap of the mode-2 grid of tz_search_kernel<1> (VTMHIP_TZ_SWITCH, default branch), four searches per workgroup:
RESUME_LISTED = 4 * RESUME_GRID   # with more listed searches its loop "for( b = blockIdx.x; b * 4 < listed; b += gridDim.x )" runs more than once
RASTER_TOT_CAP = 40 * 40          # the totals of a scan without the hint (me.hip, RASTER_TOT_CAP)
RASTER_TOT_MAX = (160 * 1024 - 1024) // 4 - 1


def raster_parts(n, max_sr=0):
    """The launcher's rule for the number of workgroups per scan, copied: min(8, 1280 / n) up to 640 searches and 1 above; at least 4 for the scans of a maxSearchRange
    hint up to 4 096 searches; 1 again when the global totals of the call (n x (totCap + 1) words) exceed 64 MB.  Returns (rasterParts, bytes of the totals)."""
    parts = min(8, 1280 // n) if n <= 640 else 1
    side = (2 * min(max_sr, 512)) // 5 + 1 if max_sr > 96 else 0
    tot_cap = min(max(side * side, RASTER_TOT_CAP), RASTER_TOT_MAX)
    if tot_cap > RASTER_TOT_CAP and n <= 4096 and parts < 4:
        parts = 4
    tot_bytes = n * (tot_cap + 1) * 4
    if parts > 1 and tot_bytes > (64 << 20):
        parts = 1
    return parts, tot_bytes


def far_start(k):
    """Start vectors 25 .. 64 samples from the motion (1/16 sample units, as test_tz_search_large_search_ranges_through_the_column_scan): the first search ends five
    samples or more from its start, so the raster scan runs"""
    return (-1) ** k * (400 + 16 * (k % 40)), (-1) ** (k // 2) * (300 + 16 * (k % 23))


def assert_rows_differ(keys, strides):
    """Generated rows, not a tiled table: at least 95 % distinct (x, y, predictor, start vector) tuples, and no row equal to the one a loop stride further on -- state
    that leaks from one pass of a workgroup's loop into the next meets another job"""
    assert len(set(keys)) * 100 >= 95 * len(keys), (len(set(keys)), len(keys))
    for s in strides:
        same = sum(1 for k in range(len(keys) - s) if keys[k] == keys[k + s])
        assert same == 0, (s, same)


@functools.lru_cache(maxsize=None)
def tz_set(n, seed, sizes, ranges, dims=(416, 240), allow_ext=True):
    """n generated jobs on the `hard` scene, fast settings off (cached-vector searches scan at distance 8 and are never listed), start vectors far from the motion,
    with the oracle's results: computed once per job set, shared by its wavesPerJob variants and never changed"""
    scene = me_util.Scene(dims[0], dims[1], hard=True)
    jobs = me_util.random_tz_jobs(scene, n, seed=seed, ranges=ranges, allow_ext=allow_ext, sizes=sizes)
    for k, j in enumerate(jobs):
        j["fast"] = 0
        j["mvHor"], j["mvVer"] = far_start(k)
    return scene, jobs, me_util.run_oracle_tz(scene, jobs)


def run_tz(ctx, scene, jobs, wpj=0, max_sr=0):
    ctx.tz_prune_stats(reset=True)
    got = _run_hip(ctx, scene, jobs, wpj, max_sr)
    return got, ctx.tz_prune_stats()


def check_tz(ctx, name, scene, jobs, exp, wpj=0, max_sr=0):
    got, st = run_tz(ctx, scene, jobs, wpj, max_sr)
    bad = [k for k in range(len(jobs)) if got[k] != exp[k]]
    print("batch sizes", name, "n", len(jobs), "wpj", wpj, st, "mismatches", len(bad))
    assert not bad, (len(bad), bad[:20], [(jobs[k], got[k], exp[k]) for k in bad[:3]])
    return st


# ---- A1 / A2: the job-table entry -------------------------------------------------------------------------------------------------------------------------------
SMALL = ((8, 16), (8, 16))      # 8x8, 16x16 (and 8x16 / 16x8): the smallest jobs the column kernel lists (8-sample segments)


# Sized with the oracle alone (searches that are not under extended settings and evaluate 600 points or more: 3 613 / 9 893 of the job tables, 9 533 / 10 411 of the fused
# rows), about 15 % over each threshold.  listed on the MI355X: A1 3 726 (> 3 072), A2 10 727, A3 8x8 10 116 and 16x16 10 687 (> 8 192)
A1_JOBS, A2_JOBS, A3_ROWS = 7600, 18000, 16000


@pytest.mark.parametrize("wpj", [0, 8])
def test_more_scans_than_column_workgroups(ctx, wpj):
    """A1: 7 600 jobs of 8x8 .. 16x16 at search range 64 / 96, a job in five with extended settings (its scan runs inside the search kernel, between the listed ones).
    More than 3 072 listed scans and at most 8 192 jobs: only the column kernel's loop runs twice (wavesPerJob 8: the resume grid is one workgroup per job).
    listed on the MI355X: 3 726."""
    scene, jobs, exp = tz_set(A1_JOBS, 9100, SMALL, (64, 96))
    assert len(jobs) <= RESUME_LISTED
    assert_rows_differ([(j["x"], j["y"], j["predHor"], j["predVer"], j["mvHor"], j["mvVer"]) for j in jobs], (COLS_GRID,))
    st = check_tz(ctx, "A1", scene, jobs, exp, wpj)
    assert st["listed"] > COLS_GRID, st


def test_more_listed_searches_than_the_resume_grid(ctx):
    """A2: 18 000 jobs of 8x8 at search range 64 without extended settings, a wave per search.  More than 8 192 listed: the column kernel's loop runs three and four
    times in a workgroup, the resume launch walks the list in a bounded grid, a workgroup calling the search twice on the same LDS arrays.  listed on the MI355X: 10 727."""
    scene, jobs, exp = tz_set(A2_JOBS, 9200, ((8,), (8,)), (64,), allow_ext=False)
    assert_rows_differ([(j["x"], j["y"], j["predHor"], j["predVer"], j["mvHor"], j["mvVer"]) for j in jobs], (COLS_GRID, RESUME_LISTED))
    st = check_tz(ctx, "A2", scene, jobs, exp, 0)
    assert st["listed"] > RESUME_LISTED, st


# ---- A3: the fused entry (the one the benchmark's levels use) -------------------------------------------------------------------------------------------------------
CFG_ALL_ROWS = (CFGV[0], CFGV[1], 0, CFGV[3], CFGV[4])      # CFGV without the row sub-sampling: a 16x16 block keeps every row in its SAD, so the block-sum bound applies to it


@functools.lru_cache(maxsize=None)
def mest_set(w, h, n, cfgv):
    """n band_jobs rows of one shape (uniform all-uni rows; PUs on the picture border, predictors next to the zero vector, 0 .. 15 m_uniMvList entries among them) with
    every search range 64 / 96, no cached integer vector, the start vector far from the motion and at most two m_uniMvList entries (they are start candidates near the
    motion: of the rows with 15 of them one in eight comes to a scan, of the rows with none two in three); the oracle's records, computed once for the attached and the
    unattached run."""
    scene, jobs = band_jobs(w, h, n)
    for k, j in enumerate(jobs):
        j["searchRange"] = (64, 96)[(k // 3) % 2]
        j["cached"] = 0
        j["mv"] = far_start(k)
        j["extra"] = j["extra"][:k % 3]
    exp, exp_int = me_util.run_oracle_mest(scene, jobs, cfgv)
    return scene, jobs, exp, exp_int


def run_mest(ctx, scene, jobs, w, h, cfgv, attach):
    """The attach / run / detach sequence of test_gpu_tz_prune.run_device with the launch's cfg as a parameter: (records, integer results, statistic of the call)"""
    n = len(jobs)
    others = np.zeros(1, np.int16)
    cfg = MeCfg(cfgv[0], cfgv[1], cfgv[2], cfgv[3], cfgv[4], 0, 1, 1, 0, 0)      # uniformImv 0, uniformSquare, uniformBi 1 (all uni)
    pic = PicParams(scene.W, scene.H, 128, 10, 0)
    d_cur, d_ref, d_oth = ctx.to_device(scene.cur), ctx.to_device(scene.ref_buf), ctx.to_device(others)
    d_jobs, d_res = ctx.to_device(np.frombuffer(hip_jobs(scene, jobs, others), np.uint8)), ctx.alloc(C.sizeof(MeOut) * n)
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


@pytest.mark.parametrize("attach", [True, False])
@pytest.mark.parametrize("w,h,cfgv", [(8, 8, CFGV), (16, 16, CFG_ALL_ROWS)])
def test_fused_rows_past_both_grids(ctx, w, h, cfgv, attach):
    """A3: 16 000 uniform all-uni rows through vtmhip_xMotionEstimation_batch_dev.  The first launch is the fused tz_group_kernel (four searches per wave), the column
    kernel and the resume launch read the job records it stored; more than 8 192 listed: both loops run more than once.  With the box sums attached the bound skips or
    reduces scans inside the column kernel's loop (its `continue` past the final barrier), without them every listed scan runs whole.  On the MI355X: 8x8 listed 10 116
    (1 skipped, 781 reduced), 16x16 -- without the row sub-sampling, which the bound does not apply to -- listed 10 687 (48 skipped, 2 755 reduced).
    Not covered here: a first launch of the fused tz_search_kernel itself (32x32 and larger; 8x8 and 16x16 both take tz_group_kernel) with more than 8 192 listed -- the
    oracle's records of the 14 000 rows of 32x32 that needs take longer than a test of the suite may."""
    scene, jobs, exp, exp_int = mest_set(w, h, A3_ROWS, cfgv)
    assert_rows_differ([(j["x"], j["y"], j["mvPred"], j["mv"]) for j in jobs], (COLS_GRID, RESUME_LISTED))
    got, got_int, st = run_mest(ctx, scene, jobs, w, h, cfgv, attach)
    bad = [k for k in range(len(jobs)) if got[k] != exp[k] or got_int[k] != exp_int[k]]
    print("batch sizes A3", (w, h), "n", len(jobs), "attached" if attach else "nothing attached", st, "mismatches", len(bad))
    assert not bad, (len(bad), bad[:20], [(got[k], exp[k], got_int[k], exp_int[k], jobs[k]["searchRange"]) for k in bad[:3]])
    assert st["listed"] > RESUME_LISTED, st
    if attach:
        assert st["skipped"] + st["reduced"] > 0, st
    else:
        assert st["skipped"] == 0 and st["reduced"] == 0 and st["points_evaluated"] == st["points_total"], st


# ---- B: workgroups per scan --------------------------------------------------------------------------------------------------------------------------------------
B_CASES = [(1, 8), (2, 8), (3, 8), (161, 7), (183, 6), (214, 5), (640, 2), (641, 1)]


@pytest.mark.parametrize("n,parts", B_CASES)
def test_every_number_of_workgroups_per_scan(ctx, n, parts):
    """B: the "last workgroup to arrive picks the minimum" protocol at 8 workgroups per scan with one, two and three scans in the call (each workgroup's list stride is
    then 1 .. 3), at 7, 6 and 5, and either side of n = 640 (2 and 1).  16x16 and 64x64 jobs at search range 64 / 96: the first n of one job set; for n <= 3 the first
    n the oracle scanned (nEval >= 600: a 26 x 26 grid at least), so that the call lists something."""
    assert raster_parts(n)[0] == parts
    scene, pool, exp_pool = tz_set(641, 9300, ((16, 64), (16, 64)), (64, 96), allow_ext=False)
    pick = list(range(n))
    if n <= 3:      # a 16x16, a 64x64 and a 16x64 search
        scanned = [k for k in range(len(pool)) if exp_pool[k][4] >= 600]
        pick = [next(k for k in scanned if (pool[k]["w"], pool[k]["h"]) == s) for s in ((16, 16), (64, 64), (16, 64))][:n]
    jobs, exp = [pool[k] for k in pick], [exp_pool[k] for k in pick]
    st = check_tz(ctx, "B rasterParts %d" % parts, scene, jobs, exp, 0)
    assert st["listed"] > 0, st
    if n <= 3:
        assert st["listed"] == n, st


# ---- C: the large-scan hint and the 64 MB bound of its global totals -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,parts", [(700, 4), (720, 1)])
def test_large_scan_hint_either_side_of_the_totals_bound(ctx, n, parts):
    """C: maxSearchRange 384 (154 x 154 + 1 words of totals per scan).  700 searches: four workgroups per scan and 66.4 MB of global totals, zeroed in the call's one
    fill; 720: 68.3 MB would exceed the 64 MB bound, one workgroup per scan.  Small blocks on the 832x480 scene at search range 96 / 192 / 384."""
    got_parts, tot_bytes = raster_parts(n, 384)
    assert got_parts == parts and (tot_bytes <= (64 << 20)) == (parts == 4) and abs(tot_bytes - (64 << 20)) < (2 << 20), (got_parts, tot_bytes)
    print("batch sizes C n", n, "rasterParts", got_parts, "global totals %.1f MB" % (tot_bytes / 1e6))
    scene, pool, exp_pool = tz_set(720, 9400, SMALL, (96, 192, 384), (832, 480), allow_ext=False)
    jobs, exp = pool[:n], exp_pool[:n]
    st = check_tz(ctx, "C", scene, jobs, exp, 0, 384)
    assert sum(1 for e in exp if e[4] > 2000) >= 50      # many searches really scanned a large window (nEval counts the scan points)
    assert st["listed"] >= 50, st


# ---- D: BDOF past one launch's 65 535 PUs; DMVR refuses such a call ----------------------------------------------------------------------------------------------------
BDOF_PERIOD, PU_PER_LAUNCH = 199, 65535


def _patch_i64(rows, field, values):
    """writes one int64 field of every row of a job table held as bytes (rows: [n][sizeof] uint8)"""
    rows[:, field.offset:field.offset + 8] = np.ascontiguousarray(values, "<i8").view(np.uint8).reshape(-1, 8)


def test_bdof_second_launch(ctx):
    """D: vtmhip_bdof_batch_dev with 65 535 + 40 PUs of 8x8, prediction only: the second launch reads d_jobs + 65535.  199 distinct jobs (expectations from vo_bdof_pu)
    cycled with period 199 -- 65 535 = 329 * 199 + 64, so row 65 535 + i holds job 64 + i, not job i -- every PU with an output offset of its own; every row compared."""
    from vtm_amd import synth
    L = ol.oracle()
    W, H, M, bd = 256, 192, 48, 10
    fr = list(synth.gen_frames(W, H, 3, seed=9))
    rng = np.random.default_rng(1310)
    planes = [np.ascontiguousarray(np.pad(f, M, mode="edge")) for f in (fr[0], fr[2])]
    S, plane_sz = planes[0].shape[1], planes[0].size
    n = PU_PER_LAUNCH + 40
    base = (PredJob * BDOF_PERIOD)()
    exp = np.zeros((BDOF_PERIOD, 64), np.int16)
    for k in range(BDOF_PERIOD):
        x, y = int(rng.integers(0, (W - 8) // 4 + 1)) * 4, int(rng.integers(0, (H - 8) // 4 + 1)) * 4
        mv = [int(v) for v in rng.integers(-500, 500, 4)]
        if k % 5 == 0:
            mv[k % 4] &= ~15
        if k % 13 == 0:
            mv = [v & ~15 for v in mv]
        e = np.zeros((8, 8), np.int16)
        at = [C.c_void_p(p.ctypes.data + 2 * ((y + M) * S + x + M)) for p in planes]
        L.vo_bdof_pu(at[0], S, at[1], S, 8, 8, *mv, bd, ol.P(e), 8)
        exp[k] = e.reshape(-1)
        j = base[k]
        for l in range(2):
            j.refOff[l], j.refStride[l] = l * plane_sz + (M + y) * S + M + x, S
        j.mv[0][0], j.mv[0][1], j.mv[1][0], j.mv[1][1] = mv
        j.predStride = j.outStride = 8
        j.width, j.height, j.mode, j.bitDepth = 8, 8, 2, bd
    rows = np.ascontiguousarray(np.frombuffer(base, np.uint8).reshape(BDOF_PERIOD, C.sizeof(PredJob))[np.arange(n) % BDOF_PERIOD])
    _patch_i64(rows, PredJob.predOff, np.arange(n) * 64)
    _patch_i64(rows, PredJob.outOff, np.arange(n) * 64)
    exp_all = exp[np.arange(n) % BDOF_PERIOD]
    # a second launch that read the table from its start again would write job i's block where job 64 + i's belongs: the two differ for every i
    assert all(not np.array_equal(exp_all[i], exp_all[PU_PER_LAUNCH + i]) for i in range(40))
    launches = -(-n // PU_PER_LAUNCH)
    print("batch sizes D n", n, "launches", launches, "rows of the second", n - PU_PER_LAUNCH)
    assert launches == 2
    d_ref = ctx.to_device(np.concatenate([p.reshape(-1) for p in planes]))
    d_jobs, d_pred = ctx.to_device(rows.reshape(-1)), ctx.to_device(np.full(n * 64, 0x5a5a, np.int16))
    ctx.bdof_batch(0, d_ref.ptr, d_pred.ptr, 0, d_jobs.ptr, n, 8, 8)
    got = d_pred.to_host(np.int16).reshape(n, 64)
    for d in (d_ref, d_jobs, d_pred):
        d.free()
    bad = np.flatnonzero((got != exp_all).any(axis=1))
    assert bad.size == 0, (bad.size, bad[:20])


@pytest.mark.parametrize("chroma", [False, True])
def test_dmvr_refuses_more_than_one_launch(ctx, chroma):
    """D': 65 536 PUs through vtmhip_dmvr_batch_dev / vtmhip_dmvr_chroma_batch_dev: VTMHIP_E_INVALID and nothing launched (the outputs keep their fill bytes).  The
    table holds 65 536 valid 8x8 rows with outputs of their own, so that a call that went through would stay inside its buffers."""
    W, H, M, n = 64, 64, 160, PU_PER_LAUNCH + 1
    plane = np.zeros((H + 2 * M, W + 2 * M), np.int16)
    S = plane.shape[1]
    one = (DmvrJob * 1)()
    j = one[0]
    for l in range(2):
        j.refOff[l], j.refStride[l] = l * plane.size + (M + 16) * S + M + 16, S
    j.puX, j.puY, j.width, j.height, j.bitDepth, j.predStride, j.outStride = 16, 16, 8, 8, 10, 8, 8
    rows = np.ascontiguousarray(np.frombuffer(one, np.uint8).reshape(1, C.sizeof(DmvrJob))[np.zeros(n, np.int64)])
    _patch_i64(rows, DmvrJob.predOff, np.arange(n) * 64)
    _patch_i64(rows, DmvrJob.outOff, np.arange(n) * 64)
    rows[:, DmvrJob.mvdRow.offset:DmvrJob.mvdRow.offset + 4] = np.arange(n).astype("<i4").view(np.uint8).reshape(-1, 4)
    pic = PicParams(W, H, 128, 10, 0)
    fill, fill_mvd = np.full(n * 64, 0x5a5a, np.int16), np.full(n * 2, 0x5a5a5a5a, np.int32)
    d_ref, d_jobs = ctx.to_device(np.concatenate([plane.reshape(-1)] * 2)), ctx.to_device(rows.reshape(-1))
    d_pred, d_mvd = ctx.to_device(fill), ctx.to_device(fill_mvd)
    with pytest.raises(VtmHipError) as err:
        (ctx.dmvr_chroma_batch if chroma else ctx.dmvr_batch)(pic, 0, d_ref.ptr, d_pred.ptr, 0, d_jobs.ptr, n, 8, 8, d_mvd.ptr)
    assert err.value.status == E_INVALID, err.value
    ctx.sync()
    got, got_mvd = d_pred.to_host(np.int16), d_mvd.to_host(np.int32)
    for d in (d_ref, d_jobs, d_pred, d_mvd):
        d.free()
    assert np.array_equal(got, fill) and np.array_equal(got_mvd, fill_mvd)
