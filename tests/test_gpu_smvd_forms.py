"""GPU parity of the symmetric-MVD search (vtmhip_smvd_batch_dev, smvd.hip) on every launch form, with clipped vectors, full start lists and tied costs -- what
tests/test_gpu_smvd.py (20 .. 150 jobs per size, natural scenes, start lists of 2 .. 8) leaves unpinned:

  B1  every instantiation of the tile kernel (the 17 shapes of the entry's switch) at 8 and 10 bits, batches of 1, pusPerWave -+ 1 and an odd few dozen jobs;
  B2  the four-slot group form (batches larger than eight eight-slot waves per compute unit: what every level of a 4K picture launches) beside the eight-slot one;
  B3  clipMv inside the search: PUs at the picture corners with vectors at and beyond the limits, over reference margins of noise;
  B4  start lists of VTMHIP_SMVD_MAX_START entries (and numStart beyond: the clamp), the evaluated entries far down the list;
  B5  tied costs (constant planes, lambda 0 / tiny): the first-minimum rules of the slot reduction, the step loop and the state update decide alone;
  B6  the entry's argument checks.

Expected values come from the oracle alone (me_util.smvd_member_results "vo_", me_util.smvd_search_oracle), job by job and bit-exact, all four ops unless a case
says otherwise.  The launch form a case is about is asserted from vtmhip_smvd_launch_form -- the rule the entry itself dispatches on -- before the device runs."""
import ctypes as C
import functools

import numpy as np
import pytest

import me_util
import oracle_lib as ol
from test_gpu_smvd import hip_jobs
from vtm_amd.lib import E_INVALID, OK, PicParams, SmvdJob, VtmHipError

pytestmark = pytest.mark.gpu

GEN64, GEN256, GROUP, WORKGROUP = 0, 1, 2, 3      # VTMHIP_SMVD_KERNEL_*
DT = np.dtype(SmvdJob)


def tiles(size):
    return (size[0] // 8) * (size[1] // 8)


def tile_form(size, slots=8):
    """what a uniform batch of a tile shape launches at 8 / 10 bits (smvd.hip: smvd_tile_waves with the default VTMHIP_SMVD_G8 / G16): the group form up to eight tiles,
    one wave per PU at 16, four above"""
    t = tiles(size)
    return (GROUP, 0, slots, 64 // (slots * t)) if t <= 8 else (WORKGROUP, 1 if t == 16 else 4, 8, 1)


@functools.lru_cache(maxsize=None)
def hard_scene(bd=10):
    return me_util.SmvdScene(416, 240, hard=True, bit_depth=bd)


@functools.lru_cache(maxsize=None)
def noise_scene(bd=10):
    return me_util.SmvdNoiseMarginScene(416, 240, bit_depth=bd)


@functools.lru_cache(maxsize=None)
def flat_scene(bd=10):
    return me_util.SmvdFlatScene(416, 240, bit_depth=bd)


def num_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def job_table(scene, jobs):
    """the device's job table as a structured array (test_gpu_smvd.hip_jobs; "numStart" of a job overrides the length of its list: the clamp)"""
    table = np.frombuffer(hip_jobs(scene, jobs), DT).copy()
    for k, j in enumerate(jobs):
        if "numStart" in j:
            table["numStart"][k] = j["numStart"]
    return table


def oracle_results(scene, jobs, members=True):
    L = ol.oracle()
    return ([me_util.smvd_member_results(scene, j, L, "vo_") for j in jobs] if members else None), [me_util.smvd_search_oracle(scene, j, L) for j in jobs]


def _tup(a):
    return [tuple(v) for v in a.tolist()]


class Device:
    """the picture planes of a scene on the device; run(): the four calls of test_gpu_smvd.device_member_results on the first n rows of a job table"""

    def __init__(self, ctx, scene):
        self.ctx, self.scene = ctx, scene
        self.pic = PicParams(scene.W, scene.H, 128, scene.bd, 0)
        self.d_cur = ctx.to_device(scene.cur)
        self.d_ref = ctx.to_device(np.concatenate([scene.ref_buf.reshape(-1), scene.ref_buf2.reshape(-1)]))

    def free(self):
        self.d_cur.free()
        self.d_ref.free()

    def op(self, table, op, max_wh, uniform):
        d_jobs = self.ctx.to_device(table.view(np.uint8).reshape(-1))
        self.ctx.smvd_batch(self.pic, self.d_cur.ptr, self.d_ref.ptr, d_jobs.ptr, len(table), max_wh[0], max_wh[1], op, uniform=uniform)
        out = d_jobs.to_host(np.uint8).view(DT)
        d_jobs.free()
        return out

    def run(self, table, jobs, n, max_wh, uniform, members=True):
        t = table[:n].copy()
        mem = None
        if members:
            pc, pt, start = t["cand"][:, 0, 0], t["cand"][:, 1, 0], t["starts"][:, 0]
            t["mvCur"], t["mvTar"] = start, pt - (start - pc)
            t["predSym"][:, 0], t["predSym"][:, 1] = pc, pt
            c0 = self.op(t, 0, max_wh, uniform)["cost"]
            t["cost"] = c0 + np.array([int(j["lam"] * 6) for j in jobs[:n]], np.uint64)
            r = self.op(t, 1, max_wh, uniform)
            me = zip(_tup(r["mvCur"]), _tup(r["mvTar"]), r["cost"].tolist())
            t["cost"] = c0 + np.array([int(j["lam"] * 9) for j in jobs[:n]], np.uint64)
            t["skip"], t["mvpIdxSym"] = t["puX"] // 4 & 1, 0
            r = self.op(t, 2, max_wh, uniform)
            chk = zip(_tup(r["predSym"][:, 0]), _tup(r["predSym"][:, 1]), _tup(r["mvpIdxSym"]), r["cost"].tolist())
            mem = list(zip(c0.tolist(), me, chk))
        r = self.op(t, 3, max_wh, uniform)
        return mem, list(zip(_tup(r["mvCur"]), _tup(r["mvTar"]), _tup(r["predSym"][:, 0]), _tup(r["predSym"][:, 1]), _tup(r["mvpIdxSym"]), r["cost"].tolist()))


def check_batch(ctx, dev, name, table, jobs, exp, n, max_wh, uniform, form):
    """asserts the launch form of the call, then runs it and compares every job with the oracle's results exp = (members or None, whole block)"""
    got_form = ctx.smvd_launch_form(max_wh[0], max_wh[1], dev.scene.bd, uniform, n)
    assert got_form == form, (name, n, got_form, form)
    mem, full = dev.run(table, jobs, n, max_wh, uniform, members=exp[0] is not None)
    bad = [k for k in range(n) if full[k] != exp[1][k] or (mem is not None and mem[k] != exp[0][k])]
    print("smvd forms", name, "n", n, "form", got_form, "mismatches", len(bad))
    assert not bad, (name, n, len(bad), bad[:20], [(jobs[k], full[k], exp[1][k], mem and mem[k], exp[0] and exp[0][k]) for k in bad[:2]])


# ---- B1: every instantiation of the tile kernel -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("size", me_util.SMVD_TILE_SHAPES)
def test_every_tile_instantiation(ctx, size, bd):
    """B1: uniform batches of each of the 17 shapes (16x64 and 64x128 among them) at 8 bits (no head-room shift in the first filter pass) and 10: one job, one job
    fewer and one more than a wave holds, and an odd number that leaves the last wave partly filled."""
    scene = hard_scene(bd)
    form = tile_form(size)
    ppw = form[3]
    m = 45 if max(size) <= 32 else 15
    jobs = me_util.random_smvd_jobs(scene, m, seed=31000 + size[0] * 131 + size[1] + bd, sizes=[size])
    exp = oracle_results(scene, jobs)
    dev = Device(ctx, scene)
    for n, first in sorted({(1, m - 1), (max(1, ppw - 1), 1), (ppw + 1, 2), (m, 0)}):      # different rows of the set for the small batches
        sub = jobs[first:first + n]
        check_batch(ctx, dev, "B1 %dx%d %d bits" % (size + (bd,)), job_table(scene, sub), sub, (exp[0][first:first + n], exp[1][first:first + n]), n, size, True, form)
    dev.free()


# ---- B2: the four-slot group form -------------------------------------------------------------------------------------------------------------------------------------
def group_threshold(size, cus):
    """The launcher's rule (smvd.hip, smvd_form), copied: eight candidate slots while ceil( n / PPW_WIDE ) <= 2 * 4 * numCUs, PPW_WIDE = 64 / (8 * tiles) PUs per
    wave; four above.  Returns the largest n that still takes eight slots."""
    ppw_wide = 64 // (8 * tiles(size))
    n = 8 * cus * ppw_wide
    assert -(-n // ppw_wide) <= 8 * cus < -(-(n + 1) // ppw_wide)
    return n


@functools.lru_cache(maxsize=None)
def group_set(size, n):
    """n generated jobs of one shape on the hard scene with the oracle's results: computed once, shared by the batches either side of the threshold"""
    scene = hard_scene()
    jobs = me_util.bulk_smvd_jobs(scene, n, 32000 + size[0] * 131 + size[1], size)
    return scene, jobs, job_table(scene, jobs), oracle_results(scene, jobs)


# 32x16 and 16x32 (eight tiles: one PU per eight-slot wave, two per four-slot wave) take the same two forms as the six shapes of up to four tiles
@pytest.mark.parametrize("size", [(8, 8), (16, 8), (8, 16), (16, 16), (32, 8), (8, 32), (32, 16), (16, 32)])
def test_four_slot_group_form(ctx, size):
    """B2: the first `threshold` jobs of a set (still eight slots) and threshold + pusPerWave + 1 (four slots, the last wave partly filled).  The four-slot form runs
    a pass of more than four candidates -- the diamond's first round, two start vectors x four predictor pairs -- as two steps."""
    thr = group_threshold(size, num_cus())
    below, above = tile_form(size, 8), tile_form(size, 4)
    assert ctx.smvd_launch_form(size[0], size[1], 10, True, thr) == below and ctx.smvd_launch_form(size[0], size[1], 10, True, thr + 1) == above
    n = thr + above[3] + 1
    assert n % above[3] != 0
    scene, jobs, table, exp = group_set(size, n)
    keys = [(j["x"], j["y"], str(j["cands"]), str(j["starts"])) for j in jobs]
    assert len(set(keys)) * 100 >= 95 * n, (len(set(keys)), n)      # generated rows, not a tiled table
    moved = sum(1 for e in exp[1] if e[0] != e[2])
    print("smvd forms B2 %dx%d" % size, "threshold", thr, "jobs", n, "distinct", len(set(keys)), "moved off the predictor", moved)
    assert moved * 4 >= n, (moved, n)
    dev = Device(ctx, scene)
    check_batch(ctx, dev, "B2 %dx%d eight slots" % size, table, jobs, exp, thr, size, True, below)
    check_batch(ctx, dev, "B2 %dx%d four slots" % size, table, jobs, exp, n, size, True, above)
    dev.free()


# ---- B3: clipped vectors ----------------------------------------------------------------------------------------------------------------------------------------------
def clip_set(scene, size, seed=4200):
    """clip_smvd_jobs of one shape, checked: the vectors lie where the case wants them, and the limits matter -- for at least half of the jobs the oracle's whole-block
    result changes when picW, picH and ctuSize are each one larger, and for at least half when each is one smaller"""
    L = ol.oracle()
    jobs, zones = me_util.clip_smvd_jobs(scene, size, 48, seed)
    assert [sum(1 for lst, zone in zones if lst == l and (zone[1] is None) == hor) for l in (0, 1) for hor in (False, True)] == [12] * 4
    for j, (lst, zone) in zip(jobs, zones):
        lim = me_util.smvd_clip_limits(scene, j)
        vecs = j["cands"][lst] + (j["starts"] if lst == 0 else [])
        for c in range(2):
            if zone[c] is not None:
                assert all(zone[c][0] <= v[c] <= zone[c][1] for v in vecs) and zone[c][0] < lim[c][j["xy"[c]] != 0] < zone[c][1], (j, zone)
            else:
                assert all(lim[c][0] < v[c] < lim[c][1] for v in vecs), (j, zone)
        assert all(lim[c][0] < v[c] < lim[c][1] for v in j["cands"][1 - lst] for c in range(2)), j
    exp = oracle_results(scene, jobs)
    larger = sum(1 for j, e in zip(jobs, exp[1]) if me_util.smvd_search_oracle_at(scene, j, L, grow=1) != e)
    smaller = sum(1 for j, e in zip(jobs, exp[1]) if me_util.smvd_search_oracle_at(scene, j, L, grow=-1) != e)
    print("smvd forms B3 %dx%d %d bits: of %d jobs the result changes with the limits one sample out %d, one sample in %d" % (size + (scene.bd, len(jobs), larger, smaller)))
    assert larger * 2 >= len(jobs) and smaller * 2 >= len(jobs), (size, larger, smaller)
    return jobs, exp


@pytest.mark.parametrize("size", me_util.SMVD_TILE_SHAPES)
def test_clipped_vectors_tile_kernel(ctx, size):
    """B3: 48 corner PUs per tile shape, uniform, 10 bits (tile_eval's clipMv).  With the 160-sample margin every clipped read stays inside the planes: the largest is
    128x128 at the right edge, picW + 7 + 128 + 4."""
    scene = noise_scene()
    jobs, exp = clip_set(scene, size)
    dev = Device(ctx, scene)
    check_batch(ctx, dev, "B3 %dx%d" % size, job_table(scene, jobs), jobs, exp, len(jobs), size, True, tile_form(size))
    dev.free()


@pytest.mark.parametrize("bd,sizes,kernel", [(10, ((16, 4), (4, 16), (4, 32)), GEN64), (12, ((16, 16), (64, 64)), GEN256)])
def test_clipped_vectors_general_kernel(ctx, bd, sizes, kernel):
    """B3: mixed batches through smvd_kernel (predict()'s clipMv): 16x4, 4x16 and 4x32 under a 16x32 hint (64 lanes), 12-bit 16x16 and 64x64 under 64x64 (256 lanes)"""
    scene = noise_scene(bd)
    jobs, mem, full = [], [], []
    for size in sizes:
        js, exp = clip_set(scene, size, 4300)
        jobs, mem, full = jobs + js, mem + exp[0], full + exp[1]
    order = np.random.default_rng(43).permutation(len(jobs)).tolist()      # the shapes mixed
    jobs, exp = [jobs[k] for k in order], ([mem[k] for k in order], [full[k] for k in order])
    hint = (max(s[0] for s in sizes), max(s[1] for s in sizes))
    dev = Device(ctx, scene)
    check_batch(ctx, dev, "B3 general %d bits" % bd, job_table(scene, jobs), jobs, exp, len(jobs), hint, False, (kernel, 0, 0, 0))
    dev.free()


# ---- B4 / B5: one job set per launch form -------------------------------------------------------------------------------------------------------------------------------
# (shape, bit depth, jobs, form of the plain batch, form of the batch repeated past the B2 threshold or None)
FORM_CASES = [((8, 8), 10, 200, tile_form((8, 8)), tile_form((8, 8), 4)),                # group form, eight PUs per wave / four slots, four PUs per wave
              ((32, 16), 10, 200, tile_form((32, 16)), tile_form((32, 16), 4)),          # group form at eight tiles: one PU per wave / four slots, two per wave
              ((32, 32), 10, 200, tile_form((32, 32)), None),                            # one wave per PU
              ((64, 64), 10, 100, tile_form((64, 64)), None),                            # four waves per PU
              ((16, 4), 10, 200, (GEN64, 0, 0, 0), None),
              ((64, 64), 12, 100, (GEN256, 0, 0, 0), None)]
FORM_IDS = ["8x8-group", "32x16-group", "32x32-wave", "64x64-four-waves", "16x4-general-64", "64x64-12bit-general-256"]


def check_forms(ctx, name, scene, size, jobs, exp, form, form_above):
    """the job set as one uniform batch, and -- for the group shapes -- repeated to threshold + pusPerWave + 1 rows, which takes the four-slot form (row k holds job
    k mod len(jobs); the whole block only)"""
    table = job_table(scene, jobs)
    dev = Device(ctx, scene)
    check_batch(ctx, dev, name, table, jobs, exp, len(jobs), size, True, form)
    if form_above:
        n = group_threshold(size, num_cus()) + form_above[3] + 1
        rows = np.arange(n) % len(jobs)
        check_batch(ctx, dev, name + " repeated", table[rows], [jobs[k] for k in rows], (None, [exp[1][k] for k in rows]), n, size, True, form_above)
    dev.free()


def long_list_conditions(scene, name, jobs, exp_full):
    """every job evaluates a raw entry of index 8 or higher; for a quarter of the jobs at least the oracle's result differs from its result with the list cut at 8"""
    L = ol.oracle()
    assert all(len(j["starts"]) == me_util.SMVD_MAX_START for j in jobs) and sum(1 for j in jobs if j.get("numStart", 0) > me_util.SMVD_MAX_START) * 5 >= len(jobs)
    assert all(max(me_util.smvd_evaluated_starts(j), default=0) >= 8 for j in jobs)
    differ = sum(1 for j, e in zip(jobs, exp_full) if me_util.smvd_search_oracle_at(scene, j, L, max_start=8) != e)
    print("smvd forms B4", name, "of %d jobs %d differ from the search with the list cut at 8 entries" % (len(jobs), differ))
    assert differ * 4 >= len(jobs), (name, differ, len(jobs))


@pytest.mark.parametrize("size,bd,n,form,form_above", FORM_CASES, ids=FORM_IDS)
def test_long_start_lists(ctx, size, bd, n, form, form_above):
    """B4: 18 start entries (bits 8 .. 17 of the tile kernel's startMask, next_start past entry 7, the "fewer than 5 distinct" stop with 6 .. 10 duplicates in front
    of the entries that count), a job in four with numStart 19 .. 22"""
    scene = hard_scene(bd)
    jobs = me_util.long_start_smvd_jobs(scene, n, 33000 + size[0] * 131 + size[1] + bd, size)
    exp = oracle_results(scene, jobs)
    long_list_conditions(scene, "%dx%d %d bits" % (size + (bd,)), jobs, exp[1])
    check_forms(ctx, "B4 %dx%d %d bits" % (size + (bd,)), scene, size, jobs, exp, form, form_above)


def test_long_start_lists_four_slot_form_generated(ctx):
    """B4: 8x8 above the B2 threshold with generated rows: the positions, predictors and settings of the B2 set under long start lists (whole block only)"""
    size = (8, 8)
    form = tile_form(size, 4)
    n = group_threshold(size, num_cus()) + form[3] + 1
    scene, base, _, _ = group_set(size, n)
    jobs = me_util.long_start_smvd_jobs(scene, n, 34000, size, base=base)
    assert all(max(me_util.smvd_evaluated_starts(j), default=0) >= 8 for j in jobs)
    exp = oracle_results(scene, jobs, members=False)
    dev = Device(ctx, scene)
    check_batch(ctx, dev, "B4 8x8 four slots", job_table(scene, jobs), jobs, exp, n, size, True, form)
    dev.free()


def tie_set(scene, size, n, seed):
    """Generated jobs on constant planes.  Even jobs: long start lists with motionLambda 0 (every cost of a pass ties), 0.01 (every rate rounds to 0) and 0.06 (rates
    of 0, 1, 2: wide ties) -- nothing is ever strictly better than the first candidate.  Odd jobs: motionLambda 1 (cost = the common distortion + the bits), index bits
    that make the second list-0 predictor's pairs far cheaper than the first pair, and start vectors a few AMVR units further from a list-0 predictor than the
    refinement can walk: several start candidates, and several directions of a diamond round, tie BELOW the cost so far (the bits of a component are constant over
    [2^k, 2^(k+1)): diagonally off the predictor the three directions towards it cost the same, and they sit in different steps of the four-slot form).  The pick
    among them is kept, the search goes on from it and -- since it cannot reach the predictor, where every path would end -- the final vector depends on it."""
    rng = np.random.default_rng(seed + 5)
    jobs = me_util.long_start_smvd_jobs(scene, n, seed, size)
    for k, j in enumerate(jobs):
        j["lam"] = (0.0, 0.01, 0.06)[k // 2 % 3]
        if k % 2:
            unit = 1 << me_util.AMVR_SHIFT[j["imv"]]
            j["lam"], j["idxBits"], j["num"] = 1.0, [[30, 1], [31, 2], [29, 1]][k // 2 % 3], [2, 2]
            c = j["cands"][0]
            if c[0] == c[1]:
                c[1] = (c[0][0] + 8 * unit, c[0][1] - 6 * unit)
            reach = 2 * (8 >> j["imv"]) + 2      # AMVR units per component the refinement cannot cover (two per diamond round, one in the cross round)
            near = [tuple(int(v + s * (reach + d) * unit) for v, s, d in zip(c[int(rng.integers(0, 4) != 0)], rng.choice([-1, 1], 2), rng.integers(0, 4, 2)))
                    for _ in range(me_util.SMVD_MAX_START)]
            j["starts"] = j["starts"][:j["numFixed"] - 1] + near[j["numFixed"] - 1:]
    return jobs


@pytest.mark.parametrize("size,bd,n,form,form_above", FORM_CASES, ids=FORM_IDS)
def test_tied_costs(ctx, size, bd, n, form, form_above):
    """B5: original and both reference planes constant: every candidate's distortion is the same, so the reference's visiting order decides -- the slot reduction's
    "lower slot on equal cost", the step loop's "earlier step on a tie" and the strict `c < cost` of the state update"""
    L = ol.oracle()
    scene = flat_scene(bd)
    n = n * 3 // 5
    jobs = tie_set(scene, size, n, 35000 + size[0] * 131 + size[1] + bd)
    exp = oracle_results(scene, jobs)
    tied = 0
    for j, e in zip(jobs, exp[1]):
        pairs, starts = me_util.smvd_tie_counts(scene, j, L)
        tied += pairs >= 2 or starts >= 2
        if j["lam"] == 0.0:      # nothing is ever strictly better: the first predictor pair, and the search never leaves it
            assert e[4] == (0, 0) and e[0] == tuple(j["cands"][0][0]) and e[1] == tuple(j["cands"][1][0]), (j, e)
    left = sum(1 for e in exp[1][1::2] if e[0] != e[2] and e[4] != (0, 0))      # odd jobs that took a start vector of the cheaper predictor and end off it
    print("smvd forms B5 %dx%d %d bits: %d of %d jobs with two or more predictor pairs or start candidates of equal least cost, %d of %d odd jobs end off their "
          "predictor" % (size + (bd, tied, n, left, n // 2)))
    assert tied * 2 >= n and left * 2 >= n // 2, (tied, left, n)
    check_forms(ctx, "B5 %dx%d %d bits" % (size + (bd,)), scene, size, jobs, exp, form, form_above)


# ---- B6: arguments ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_arguments(ctx):
    """B6: bit depths 7 and 13, sizes that are no multiple of 4 or above 128, op 4: VTMHIP_E_INVALID from the search and from the form entry, nothing launched (the job
    table keeps its bytes); n = 0 with null pointers is a no-op"""
    scene = hard_scene()
    jobs = me_util.random_smvd_jobs(scene, 8, seed=36000, sizes=[(8, 8)])
    table = job_table(scene, jobs)
    table["cost"] = 0x5a5a5a5a5a5a5a5a
    raw = table.view(np.uint8).reshape(-1)
    dev = Device(ctx, scene)
    d_jobs = ctx.to_device(raw)
    pic = lambda bd: PicParams(scene.W, scene.H, 128, bd, 0)      # noqa: E731
    search = lambda bd, org, n, w, h, op: ctx.L.vtmhip_smvd_batch_dev(ctx.h, C.byref(pic(bd)), org, dev.d_ref.ptr, d_jobs.ptr, n, w, h, op)      # noqa: E731
    for bd, w, h, op in ((7, 8, 8, 3), (13, 8, 8, 3), (10, 6, 8, 3), (10, 8, 10, 0), (10, 132, 8, 3), (10, 8, 256, 1), (10, 0, 8, 2), (10, 8, 8, 4), (10, 8, 8, -1)):
        for uniform in (0, 0x100):
            assert search(bd, dev.d_cur.ptr, len(jobs), w, h, op | uniform) == E_INVALID, (bd, w, h, op, uniform)
            if 0 <= op <= 3:
                with pytest.raises(VtmHipError) as err:
                    ctx.smvd_launch_form(w, h, bd, uniform != 0, len(jobs))
                assert err.value.status == E_INVALID, (bd, w, h, err.value)
    assert search(10, None, len(jobs), 8, 8, 3) == E_INVALID      # null plane with n > 0
    assert search(10, dev.d_cur.ptr, -1, 8, 8, 3) == E_INVALID
    ctx.sync()
    assert np.array_equal(d_jobs.to_host(np.uint8), raw)
    for op in range(4):
        assert ctx.L.vtmhip_smvd_batch_dev(ctx.h, C.byref(pic(10)), None, None, None, 0, 8, 8, op) == OK
    assert ctx.smvd_launch_form(8, 8, 10, True, 0) == tile_form((8, 8))
    d_jobs.free()
    dev.free()
