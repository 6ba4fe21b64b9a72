"""GPU: the GEO merge candidates on the device -- vtmhip_geo_cand_satd_batch_dev and vtmhip_geo_blend_batch_dev (vtm_amd/csrc/geo.hip) on the 256 x 192 scene of
test_gpu_mmvd.py.  The expectation is built without libvtmhip (geo_util.expect_cu: vo_mc_luma with bi = 1, vo_sad, vo_sad_mask and vo_weighted_geo_blk over planes
read with the reference's walks, vo_satd / vo_sad, the list in numpy float64); the result records, the sadLarge table and the kept blocks must be bit-identical,
with guard patterns round every output."""
import ctypes as C
import functools

import numpy as np
import pytest

import geo_util as gu
import oracle_lib as ol
import test_gpu_mmvd as tm      # the scene: original plane and two reference planes with their border
from test_gpu_ciip import hip_runtime
from vtm_amd import lib

PIC_W, PIC_H, REF_STRIDE = tm.PIC_W, tm.PIC_H, tm.REF_STRIDE
NO_COST = gu.NO_COST
GUARD = 256      # bytes of pattern in front of and behind every output
FILL = 0xA5
RES = C.sizeof(lib.GeoResult)

# one batch per value vtmhip_geo_lanes_per_job can return; the issue's shapes that fit under the batch's bound, plus the other shapes of that path
BATCHES = {
    64: [(8, 8), (16, 8), (8, 16), (32, 32), (16, 16), (32, 16), (8, 8), (16, 32), (32, 32), (8, 16)],
    256: [(64, 64), (64, 16), (16, 64), (8, 8), (32, 32), (16, 8), (64, 32), (8, 16), (32, 64), (64, 64)],
}
MAX_SIDE = {64: (32, 32), 256: (64, 64)}
NUM_CAND = [2, 3, 6, 4, 5]
MVS = [(6, -10), (-22, 13), (0, 0), (24, 8), (8, -8), (16, 32), (5, 3), (-18, 7), (40, 0), (0, -24), (-3, 11)]      # fractional, whole- and half-sample phases, mixed
LAMBDAS = [0.37 * 1.7 ** k for k in range(28)]      # 0.37 .. 6e5, none of them a dyadic fraction


def job_of(k, w, h):
    x, y = (k * 24) % (PIC_W - w + 1) & ~3, (k * 40) % (PIC_H - h + 1) & ~3
    nc = NUM_CAND[k % 5]
    cands = [dict(list=(k + c) & 1, mv=MVS[(3 * k + c) % len(MVS)], keep=(k + c) % 3 == 0) for c in range(nc)]
    return dict(w=w, h=h, x=x, y=y, num_cand=nc, regime=k % 3, cands=cands)


def predict(L, refs, job, c, bd):
    e = np.zeros((job["h"], job["w"]), np.int16)
    at = C.c_void_p(refs.ctypes.data + 2 * tm.ref_off(c["list"], job["x"], job["y"]))
    L.vo_mc_luma(at, REF_STRIDE, job["w"], job["h"], c["mv"][0], c["mv"][1], 1, bd, 0, ol.P(e), job["w"])
    return e


class Batch:
    """jobs with their kept slots laid out, and what the device must leave: per job the expectation of geo_util.expect_cu and the kept plane"""

    def __init__(self, shapes, bd, jobs=None, lambdas=None):
        L = ol.oracle()
        self.bd, self.org, self.refs = bd, *tm.scene(bd)
        self.planes, self.masks = gu.weight_planes(), gu.mask_planes()
        self.jobs = [job_of(k, w, h) for k, (w, h) in enumerate(shapes)] if jobs is None else jobs
        self.exp, kept = [], 0
        for i, job in enumerate(self.jobs):
            w, h = job["w"], job["h"]
            job["preds"] = [predict(L, self.refs, job, c, bd) for c in job["cands"]]
            job["org"] = np.ascontiguousarray(self.org[job["y"]:job["y"] + h, job["x"]:job["x"] + w])
            job["sads"] = gu.expect_sads(L, job["org"], job["preds"], w, h, bd, self.masks)
            if lambdas is not None:
                job["lam"] = lambdas[i]
            elif "lam" not in job:
                job["lam"] = self.pick_lambda(job)
            for c in job["cands"]:
                c["keep_off"] = kept if c["keep"] else -1      # relative to the kept plane
                kept += w * h
        self.kept_samples = kept

    @staticmethod
    def pick_lambda(job):
        want = job["regime"]
        for lam in LAMBDAS:
            n = len(gu.expect_list(*job["sads"], job["num_cand"], lam))
            if (n == 0, 0 < n < 60, n > 60)[want]:
                return lam
        return LAMBDAS[0]

    def expect(self, ok=None):
        """ok[i] == False: job i is malformed and must be skipped"""
        L = ol.oracle()
        self.kept = np.full(self.kept_samples, FILL * 0x0101, np.uint16).view(np.int16)
        for i, job in enumerate(self.jobs):
            if ok is not None and not ok[i]:
                self.exp.append(None)
                continue
            self.exp.append(gu.expect_cu(L, job["org"], job["preds"], job["w"], job["h"], self.bd, job["num_cand"], job["lam"], self.planes, self.masks, sads=job["sads"]))
            for c, p in zip(job["cands"], job["preds"]):
                if c["keep_off"] >= 0:
                    self.kept[c["keep_off"]:c["keep_off"] + p.size] = p.reshape(-1)
        self.kept.setflags(write=False)
        return self

    def result_bytes(self, use_satd, reps=1):
        one = b"".join(bytes(gu.result_struct(e, use_satd)) for e in self.exp)
        return np.frombuffer(one * reps, np.uint8)

    def split_table(self, reps=1):
        one = np.concatenate([np.full((64, 6), NO_COST, np.uint64) if e is None else e["large"] for e in self.exp])
        return np.tile(one.reshape(-1), reps)


@functools.lru_cache(maxsize=None)
def expectation(lanes, bd):
    """computed once per (path, depth), shared and left unchanged"""
    return Batch(BATCHES[lanes], bd).expect()


def to_struct(job, bd, keep_at=None, org_stride=PIC_W):
    cands = [(tm.ref_off(c["list"], job["x"], job["y"]), c.get("ref_stride", REF_STRIDE), c["mv"][0], c["mv"][1],
              keep_at + c["keep_off"] if (keep_at is not None and c["keep_off"] >= 0) else -1) for c in job["cands"]]
    s = gu.geo_job(job.get("sw", job["w"]), job.get("sh", job["h"]), job.get("sbd", bd), job.get("snum", job["num_cand"]), job.get("slam", job["lam"]),
                   org_off=job["y"] * PIC_W + job["x"], org_stride=job.get("sorg_stride", org_stride), cands=cands[:6])
    return s


def run_device(ctx, b, lanes, use_satd, reps=1, n=None, launch=None, with_pred=True, with_split=True):
    """-> (result bytes [n * RES], sadSplit [n * 384] or None, the kept plane's samples, guards intact)"""
    keep_at = GUARD // 2
    structs = []
    for r in range(reps):
        for job in b.jobs:
            structs.append(to_struct(job, b.bd, keep_at + r * b.kept_samples if with_pred else None))
    n = len(structs) if n is None else n
    table = np.frombuffer((lib.GeoJob * len(structs))(*structs), np.uint8).copy()
    pred = np.full(GUARD // 2 + reps * b.kept_samples + GUARD // 2, FILL * 0x0101, np.uint16).view(np.int16)
    d_ref, d_org, d_pred, d_jobs = (ctx.to_device(a) for a in (b.refs, b.org, pred, table))
    d_res = ctx.to_device(np.full(n * RES + 2 * GUARD, FILL, np.uint8))
    d_split = ctx.to_device(np.full(n * 384 * 8 + 2 * GUARD, FILL, np.uint8))
    mw, mh = MAX_SIDE[lanes]
    try:
        call = lambda: ctx.geo_cand_satd_batch(d_ref.ptr, d_org.ptr, d_pred.ptr if with_pred else None, d_jobs.ptr, n, mw, mh, d_res.ptr + GUARD,      # noqa: E731
                                               d_split.ptr + GUARD if with_split else None, use_satd=use_satd)
        call() if launch is None else launch(call)
        ctx.sync()
        raw_r, raw_s, raw_p = d_res.to_host(np.uint8), d_split.to_host(np.uint8), d_pred.to_host(np.int16)
    finally:
        for buf in (d_ref, d_org, d_pred, d_jobs, d_res, d_split):
            buf.free()
    fill = np.uint16(FILL * 0x0101).view(np.int16)
    guards = bool((raw_r[:GUARD] == FILL).all() and (raw_r[GUARD + n * RES:] == FILL).all() and (raw_s[:GUARD] == FILL).all() and (raw_s[GUARD + n * 3072:] == FILL).all() and
                  (raw_p[:keep_at] == fill).all() and (raw_p[keep_at + reps * b.kept_samples:] == fill).all())
    if not with_split:
        guards = guards and bool((raw_s == FILL).all())
    return raw_r[GUARD:GUARD + n * RES].copy(), raw_s[GUARD:GUARD + n * 3072].view(np.uint64).copy(), raw_p[keep_at:keep_at + reps * b.kept_samples].copy(), guards


def explain(b, use_satd, res):
    """the first job whose record differs, field by field, for the assertion message"""
    got = (lib.GeoResult * len(b.exp)).from_buffer_copy(res.tobytes())
    for i, e in enumerate(b.exp):
        want = gu.result_struct(e, use_satd)
        if bytes(want) != bytes(got[i]):
            g, x = got[i], want
            return (i, (b.jobs[i]["w"], b.jobs[i]["h"]), b.jobs[i]["num_cand"], "whole", list(g.sadWhole), list(x.sadWhole), "passed", g.numPassed, x.numPassed,
                    "first rows", gu.result_rows(g)[:3], gu.result_rows(x)[:3])
    return None


def check_expectation(lanes, bd):
    """the expectation depends on what the kernel must get right (CPU only): each mirror case, the height >= width offset branch, the filter threshold, the cap"""
    L = ol.oracle()
    b = expectation(lanes, bd)
    seen = dict(mirror0=0, mirror1=0, mirror2=0, tall_branch=0, wide_branch=0, threshold=0, cap=0, kept=0, unkept=0)
    regimes = set()
    for job, e in zip(b.jobs, b.exp):
        w, h, nc = job["w"], job["h"], job["num_cand"]
        regimes.add(0 if e["num_passed"] == 0 else 1 if e["num_passed"] < 60 else 2)
        args = (L, job["org"], job["preds"], w, h, bd, nc, job["lam"], b.planes, b.masks)
        seen["kept"] += sum(c["keep_off"] >= 0 for c in job["cands"])
        seen["unkept"] += sum(c["keep_off"] < 0 for c in job["cands"])
        if e["num_passed"] > 60:
            seen["cap"] += len(gu.expect_cu(*args, sads=job["sads"], cap=61)["rows"]) == 61 and len(e["rows"]) == 60
        # the threshold: a shift of it by the gap to the nearest sum on either side changes the count
        if e["num_passed"] > 0:
            seen["threshold"] += len(gu.expect_list(*job["sads"], nc, job["lam"], threshold_shift=-1.0e9)) == 0 and \
                len(gu.expect_list(*job["sads"], nc, job["lam"], threshold_shift=1.0e9)) == 64 * nc * (nc - 1) != e["num_passed"]
        # a listed split of each mirror case / offset branch, blended as if it were not mirrored / took the other branch, gives another block
        def unmirrored(split, bw, bh, chroma):
            mi = gu.blend_walk(split, bw, bh, chroma)[0]
            ox, oy = gu.weight_offset(split, bw, bh)
            return mi, oy * gu.M + ox, 1, gu.M

        def other_branch(split, bw, bh, chroma):
            return gu.blend_walk(split, bh, bw, chroma)

        if not e["rows"] or all(seen[k] for k in ("mirror0", "mirror1", "mirror2", "tall_branch", "wide_branch")):
            continue
        one = gu.expect_cu(*args, sads=job["sads"], walk=unmirrored)
        other = gu.expect_cu(*args, sads=job["sads"], walk=other_branch) if w != h else None
        for t, ((s, c0, c1, bits, d), blk) in enumerate(zip(e["rows"], e["blends"])):
            a, dist = gu.SPLITS[s]
            mir = gu.ANGLE2MIRROR[a]
            assert one["rows"][t][:4] == (s, c0, c1, bits)      # the walk does not touch the list
            if mir == 0:
                seen["mirror0"] += np.array_equal(one["blends"][t], blk)
            else:
                seen["mirror%d" % mir] += not np.array_equal(one["blends"][t], blk)
            if other is not None and dist > 0 and a % 16 not in (0, 8):
                seen["tall_branch" if h >= w else "wide_branch"] += not np.array_equal(other["blends"][t], blk)
    assert all(v > 0 for v in seen.values()), (lanes, bd, seen)
    assert regimes == {0, 1, 2}, regimes
    assert {j["num_cand"] for j in b.jobs} == {2, 3, 4, 5, 6}
    assert {(c["mv"][0] & 15 != 0, c["mv"][1] & 15 != 0) for j in b.jobs for c in j["cands"]} == {(False, False), (True, False), (False, True), (True, True)}
    return seen


def test_batches_hold_the_shapes_the_kernel_can_go_wrong_at():
    assert {(8, 8), (16, 8), (8, 16), (32, 32)} <= set(BATCHES[64]) and {(8, 8), (16, 8), (8, 16), (32, 32), (64, 16), (16, 64), (64, 64)} <= set(BATCHES[256])
    L = lib.load()
    for lanes, shapes in BATCHES.items():
        assert L.vtmhip_geo_lanes_per_job(*MAX_SIDE[lanes]) == lanes
        assert all(w <= MAX_SIDE[lanes][0] and h <= MAX_SIDE[lanes][1] and (w, h) in gu.SHAPES for w, h in shapes)
        assert max(w * h for w, h in shapes) == MAX_SIDE[lanes][0] * MAX_SIDE[lanes][1]


def test_expectation_depends_on_what_the_kernel_must_get_right():
    """the same checks the GPU test makes before it asks the device, on the smaller batch (CPU only)"""
    check_expectation(64, 10)


@pytest.mark.gpu
@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("lanes", [64, 256])
def test_geo_records_tables_and_kept_blocks_match_the_expectation(ctx, lanes, bd):
    check_expectation(lanes, bd)
    b = expectation(lanes, bd)
    for use_satd in (True, False):
        res, split, kept, guards = run_device(ctx, b, lanes, use_satd)
        assert guards, "a write outside the result table / the sadLarge table / the kept plane"
        assert np.array_equal(split, b.split_table()), (lanes, bd)
        assert np.array_equal(res, b.result_bytes(use_satd)), explain(b, use_satd, res)
        assert np.array_equal(kept, b.kept), (lanes, bd)      # kept blocks exact, unkept slots still the pattern
    res, split, kept, guards = run_device(ctx, b, lanes, True, with_split=False)      # d_sadSplit is optional
    assert guards and np.array_equal(res, b.result_bytes(True))


def malformed_batch(bd):
    """the 64-lane batch with one field broken per job: every clause of the predicate but the missing d_predBase, and four untouched neighbours"""
    jobs = [job_of(k, w, h) for k, (w, h) in enumerate(BATCHES[64])]
    for j in jobs:
        j["lam"] = 0.37
    jobs[0]["sw"] = 4                        # a side outside the set
    jobs[1]["sw"], jobs[1]["sh"] = 64, 8     # 64 x 8: w < 8h fails (and above the batch's bound)
    jobs[3]["sw"] = 64                       # 64 x 32: a GEO shape, above maxWidth
    jobs[4]["sbd"] = 13
    jobs[5]["snum"] = 1
    jobs[6]["snum"] = 7
    jobs[7]["sorg_stride"] = jobs[7]["w"] - 1
    jobs[8]["cands"][1]["ref_stride"] = jobs[8]["w"] - 1
    jobs[9]["slam"] = float("nan")
    ok = [i == 2 for i in range(10)]
    extra = [job_of(10 + k, w, h) for k, (w, h) in enumerate([(16, 16), (8, 8), (32, 16), (8, 16), (16, 8)])]
    for j in extra:
        j["lam"] = 0.37
    extra[1]["slam"], extra[3]["slam"] = -1.0, float("inf")
    extra[2]["sbd"] = 7
    ok += [True, False, False, False, True]
    return Batch(None, bd, jobs=jobs + extra).expect(ok), ok


@pytest.mark.gpu
def test_malformed_jobs_are_skipped_alone(ctx):
    b, ok = malformed_batch(10)
    assert sum(ok) == 3 and any(c["keep_off"] >= 0 for i, j in enumerate(b.jobs) if not ok[i] for c in j["cands"])      # skipped jobs that asked for a kept block
    for use_satd in (True, False):
        res, split, kept, guards = run_device(ctx, b, 64, use_satd)
        assert guards
        assert np.array_equal(res, b.result_bytes(use_satd)), explain(b, use_satd, res)
        assert np.array_equal(split, b.split_table()) and np.array_equal(kept, b.kept)
    # a keepOff >= 0 without d_predBase: that job alone is skipped
    pair = [dict(j, cands=[dict(c) for c in j["cands"]]) for j in (b.jobs[10], b.jobs[14])]
    for j, keeps in zip(pair, ([False] * 6, [True] + [False] * 5)):
        for c, k in zip(j["cands"], keeps):
            c["keep"] = k
    plain = Batch(None, 10, jobs=pair).expect([True, False])
    structs = [to_struct(plain.jobs[0], 10, None), to_struct(plain.jobs[1], 10, 0)]
    assert structs[1].cand[0].keepOff >= 0 and all(structs[0].cand[k].keepOff == -1 for k in range(6))
    table = np.frombuffer((lib.GeoJob * 2)(*structs), np.uint8).copy()
    d = [ctx.to_device(a) for a in (plain.refs, plain.org, table, np.full(2 * RES, FILL, np.uint8))]
    try:
        ctx.geo_cand_satd_batch(d[0].ptr, d[1].ptr, None, d[2].ptr, 2, 32, 32, d[3].ptr)
        ctx.sync()
        assert np.array_equal(d[3].to_host(np.uint8), plain.result_bytes(True)), "a job with a kept block and no d_predBase must be skipped, its neighbour not"
    finally:
        for buf in d:
            buf.free()


@pytest.mark.gpu
def test_wrong_bounds_fail_before_anything_runs(ctx):
    buf = ctx.to_device(np.zeros(4096, np.uint8))
    try:
        for mw, mh in ((64, 8), (4, 4), (128, 128), (24, 8)):
            with pytest.raises(lib.VtmHipError) as e:
                ctx.geo_cand_satd_batch(buf.ptr, buf.ptr, buf.ptr, buf.ptr, 1, mw, mh, buf.ptr)
            assert e.value.status == lib.E_INVALID
        ctx.geo_cand_satd_batch(buf.ptr, buf.ptr, buf.ptr, buf.ptr, 0, 8, 8, buf.ptr)      # an empty batch is a no-op
        ctx.geo_blend_batch(buf.ptr, buf.ptr, buf.ptr, 0)
    finally:
        buf.free()


@pytest.mark.gpu
def test_ties_come_out_in_the_stated_order(ctx):
    """duplicate candidates (one vector on one list, three times) and lambda 0: every combination of a split ties; the device against vtmhip_geo_host"""
    bd = 10
    jobs = []
    for k, (w, h) in enumerate([(8, 8), (16, 8), (32, 32), (16, 16)]):
        j = job_of(k, w, h)
        j["num_cand"], j["lam"] = 3, 0.0 if k != 3 else 0.1
        j["cands"] = [dict(list=0, mv=(6, -10), keep=False) for _ in range(3)]
        if k >= 2:
            j["cands"][2] = dict(list=1, mv=(-22, 13), keep=False)      # two equal candidates among three
        jobs.append(j)
    b = Batch(None, bd, jobs=jobs).expect()
    res, split, kept, guards = run_device(ctx, b, 64, True)
    assert guards
    got = (lib.GeoResult * len(jobs)).from_buffer_copy(res.tobytes())
    L = lib.load()
    for i, job in enumerate(jobs):
        st, host, hsplit, _ = gu.host_job(L, gu.geo_job(job["w"], job["h"], bd, 3, job["lam"]), job["org"], job["preds"])
        assert st == 0 and bytes(host) == bytes(got[i]), (i, gu.result_rows(got[i])[:8], gu.result_rows(host)[:8])
        assert np.array_equal(split[i * 384:(i + 1) * 384].reshape(64, 6), hsplit)
        rows = gu.result_rows(got[i])[:got[i].numTested]
        keys = [(r[3], r[0], gu.PAIRS.index((r[1], r[2]))) for r in rows]
        assert keys == sorted(keys) and len(set(keys)) == len(keys)      # ascending by cost, then splitDir, then pair order
        assert i >= 2 or len({r[3] for r in rows}) < len(rows)           # and ties do occur
    assert [(r[0], r[1], r[2]) for r in gu.result_rows(got[0])] == [(t // 6,) + gu.PAIRS[t % 6] for t in range(60)]
    assert np.array_equal(res, b.result_bytes(True)), explain(b, True, res)


@pytest.mark.gpu
def test_long_batch_repeats_its_table(ctx):
    """a few thousand 8 x 8 CUs: the ten-job table repeated, the last repetition cut"""
    shapes = [(8, 8)] * 10
    b = Batch(shapes, 10).expect()
    base_r, base_s, base_k, guards = run_device(ctx, b, 64, True)
    assert guards and np.array_equal(base_r, b.result_bytes(True)), explain(b, True, base_r)
    reps, n = 301, 3003
    table_b = b
    keep_at = GUARD // 2
    structs = [to_struct(job, b.bd, keep_at + r * b.kept_samples) for r in range(reps) for job in b.jobs]
    table = np.frombuffer((lib.GeoJob * len(structs))(*structs), np.uint8).copy()
    pred = np.full(GUARD // 2 + reps * b.kept_samples + GUARD // 2, FILL * 0x0101, np.uint16).view(np.int16)
    d_ref, d_org, d_pred, d_jobs = (ctx.to_device(a) for a in (b.refs, b.org, pred, table))
    d_res, d_split = ctx.to_device(np.full(n * RES + 2 * GUARD, FILL, np.uint8)), ctx.to_device(np.full(n * 3072 + 2 * GUARD, FILL, np.uint8))
    try:
        ctx.geo_cand_satd_batch(d_ref.ptr, d_org.ptr, d_pred.ptr, d_jobs.ptr, n, 8, 8, d_res.ptr + GUARD, d_split.ptr + GUARD)
        ctx.sync()
        raw_r, raw_s, raw_p = d_res.to_host(np.uint8), d_split.to_host(np.uint8), d_pred.to_host(np.int16)
    finally:
        for buf in (d_ref, d_org, d_pred, d_jobs, d_res, d_split):
            buf.free()
    assert (raw_r[:GUARD] == FILL).all() and (raw_r[GUARD + n * RES:] == FILL).all() and (raw_s[:GUARD] == FILL).all() and (raw_s[GUARD + n * 3072:] == FILL).all()
    assert np.array_equal(raw_r[GUARD:GUARD + n * RES], np.tile(base_r, reps)[:n * RES])
    assert np.array_equal(raw_s[GUARD:GUARD + n * 3072].view(np.uint64), np.tile(base_s, reps)[:n * 384])
    done, fill = n // 10, np.uint16(FILL * 0x0101).view(np.int16)
    assert np.array_equal(raw_p[keep_at:keep_at + done * b.kept_samples], np.tile(table_b.kept, done))
    tail = np.full(b.kept_samples, fill, np.int16)
    for job in b.jobs[:n - done * 10]:
        for c in job["cands"]:
            if c["keep_off"] >= 0:
                tail[c["keep_off"]:c["keep_off"] + 64] = b.kept[c["keep_off"]:c["keep_off"] + 64]
    assert np.array_equal(raw_p[keep_at + done * b.kept_samples:keep_at + (done + 1) * b.kept_samples], tail)
    assert (raw_p[keep_at + (done + 1) * b.kept_samples:] == fill).all() and (raw_p[:keep_at] == fill).all()


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [64, 256])
def test_call_runs_under_a_stream_capture_and_replays(lanes):
    """captured on the context's stream in the strictest capture mode (one branch: a single launch), replayed once: the tables of the eager call.  Both
    instantiations; the 256-lane one has raised its dynamic-LDS limit in the eager call, so the captured call makes nothing but its launch"""
    from vtm_amd.device import Context
    b = expectation(lanes, 10)
    own = Context(0)
    H = hip_runtime()
    stream, graph, graph_exec = C.c_void_p(), C.c_void_p(), C.c_void_p()
    try:
        eager = run_device(own, b, lanes, True)
        assert eager[3] and np.array_equal(eager[0], b.result_bytes(True))
        assert H.hipStreamCreate(C.byref(stream)) == 0

        def launch(call):
            own.sync()                       # the uploads are done before the stream changes
            own.set_stream(stream)
            assert H.hipStreamBeginCapture(stream, 0) == 0      # hipStreamCaptureModeGlobal
            try:
                call()
            finally:
                assert H.hipStreamEndCapture(stream, C.byref(graph)) == 0
            assert H.hipGraphInstantiate(C.byref(graph_exec), graph, None, None, C.c_size_t(0)) == 0
            assert H.hipGraphLaunch(graph_exec, stream) == 0
            assert H.hipStreamSynchronize(stream) == 0
            own.use_own_stream()

        res, split, kept, guards = run_device(own, b, lanes, True, launch=launch)
        assert guards
        assert np.array_equal(res, eager[0]) and np.array_equal(split, eager[1]) and np.array_equal(kept, eager[2])
    finally:
        own.use_own_stream()
        if graph_exec:
            H.hipGraphExecDestroy(graph_exec)
        if graph:
            H.hipGraphDestroy(graph)
        if stream:
            H.hipStreamDestroy(stream)
        own.close()


# ---- the blend entry -------------------------------------------------------------------------------------------------------------------------------------------
def blend_case():
    """luma jobs over the golden cases' 14-bit blocks (the recorded blends of the first listed combinations) and chroma jobs over the recorded Cb / Cr blocks, mixed,
    with strides above the width; every fifth job is broken and must leave its destination as it is"""
    g = gu.load_golden()["cases"]
    src, jobs, exp, at, dst_at = [np.zeros(3, np.int16)], [], [], 3, 5
    rows = []
    for c in g:
        for t in range(min(len(c["blend"]), 12)):
            s, c0, c1 = c["list"][t].tolist()
            rows.append((c["w"], c["h"], c["bd"], s, 0, c["pred"][c0], c["pred"][c1], c["blend"][t]))
        for ch in c["chroma"]:
            rows.append((c["w"], c["h"], c["bd"], ch["split"], 1, ch["src0"], ch["src1"], ch["blend"]))
    rng = np.random.default_rng(9)
    breakers = [dict(width=4), dict(splitDir=64), dict(chroma=2), dict(bitDepth=13), dict(dstStride=3), dict(src0Stride=3), dict(width=64, height=8)]
    for k, (w, h, bd, s, chroma, s0, s1, out) in enumerate(rows):
        bw, bh = w >> chroma, h >> chroma
        pad0, pad1, padd = k % 3, (k + 1) % 4, (k + 2) % 5
        pools = []
        for blk, pad in ((s0, pad0), (s1, pad1)):
            pool = rng.integers(-8192, 8191, (bh, bw + pad)).astype(np.int16)
            pool[:, :bw] = blk
            pools.append(pool)
        j = lib.GeoCuBlendJob()
        j.src0Off, j.src1Off, j.dstOff = at, at + pools[0].size, dst_at
        j.src0Stride, j.src1Stride, j.dstStride, j.width, j.height, j.splitDir, j.chroma, j.bitDepth = bw + pad0, bw + pad1, bw + padd, w, h, s, chroma, bd
        good = k % 5 != 4
        if not good:
            for name, v in breakers[(k // 5) % len(breakers)].items():
                setattr(j, name, v)
        src += [pools[0].reshape(-1), pools[1].reshape(-1)]
        at += pools[0].size + pools[1].size
        jobs.append(j)
        exp.append((dst_at, bw, bh, bw + padd, out if good else None))
        dst_at += bh * (bw + padd) + 7
    return np.concatenate(src), jobs, exp, dst_at


def test_blend_case_holds_luma_chroma_and_broken_jobs():
    src, jobs, exp, size = blend_case()
    assert {j.chroma for j in jobs} >= {0, 1} and sum(e[4] is None for e in exp) >= 7 and {j.bitDepth for j in jobs} >= {8, 10, 12}
    assert {gu.ANGLE2MIRROR[gu.SPLITS[j.splitDir][0]] for j in jobs if j.splitDir < 64} == {0, 1, 2}


@pytest.mark.gpu
def test_blend_entry_against_the_recorded_blocks(ctx):
    src, jobs, exp, size = blend_case()
    table = np.frombuffer((lib.GeoCuBlendJob * len(jobs))(*jobs), np.uint8).copy()
    dst = np.full(size + GUARD, FILL * 0x0101, np.uint16).view(np.int16)
    fill = dst[0]
    d_src, d_dst, d_jobs = ctx.to_device(src), ctx.to_device(dst), ctx.to_device(table)
    try:
        ctx.geo_blend_batch(d_src.ptr, d_dst.ptr, d_jobs.ptr, len(jobs))
        ctx.sync()
        got, src_after = d_dst.to_host(np.int16), d_src.to_host(np.int16)
    finally:
        for buf in (d_src, d_dst, d_jobs):
            buf.free()
    assert np.array_equal(src_after, src)
    want = dst.copy()
    for at, bw, bh, stride, out in exp:
        if out is not None:
            view = want[at:at + bh * stride].reshape(bh, stride)
            view[:, :bw] = out
    assert np.array_equal(got, want), [k for k, (at, bw, bh, stride, out) in enumerate(exp) if not np.array_equal(got[at:at + bh * stride], want[at:at + bh * stride])][:5]
    assert (got[size:] == fill).all()
