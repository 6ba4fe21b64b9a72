"""GPU: vtmhip_mmvd_cand_satd_batch_dev against an expectation built without the library -- the candidates by mmvd_util, the predictions by the oracle (vo_mc_luma,
vo_add_avg, vo_add_weighted_avg, vo_bdof_pu), the costs by vo_satd / vo_sad.  Records and costs must be bit-identical, every one of a job's 64 costs on its own.

One batch per lane path of vtmhip_mc_lanes_per_block (8, 16, 64, 256 lanes), 8-, 10- and 12-bit samples, SATD and SAD.  Before the device is asked, the expectation
itself is shown to depend on what the kernel must get right (check_expectation): the scaled second offset on either list and the long-term mirror, BDOF against the
plain average and the step rule, the alternative half-sample filter, the BCW weights, the clipped prediction vectors.  The other route (VTMHIP_MMVD_FUSED=0 / 1, read once
per process: a child process) must leave identical tables; a malformed table is rejected with the outputs untouched."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    for p in (ROOT, os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)

import mmvd_util as mu      # noqa: E402
import oracle_lib as ol     # noqa: E402

PIC_W, PIC_H, CTU, MARGIN, SLACK = 256, 192, 128, 160, 2048
REF_STRIDE = PIC_W + 2 * MARGIN
PLANE = (PIC_H + 2 * MARGIN) * REF_STRIDE
NO_COST = (1 << 64) - 1
GUARD = 256      # bytes in front of and behind each output table

# (config, width, height) per job; the configs are those of job_of()
BATCHES = {
    8: [(0, 8, 8), (1, 8, 8), (2, 8, 8), (3, 8, 8), (4, 8, 8), (5, 8, 4), (6, 4, 8), (7, 8, 8), (1, 8, 4), (0, 4, 8), (5, 8, 8)],
    16: [(0, 16, 8), (1, 8, 16), (2, 16, 16), (3, 16, 16), (4, 16, 8), (5, 16, 16), (6, 8, 16), (7, 8, 8), (0, 8, 4), (3, 4, 8), (0, 16, 16)],
    64: [(0, 32, 32), (1, 32, 32), (2, 32, 16), (3, 32, 32), (4, 16, 16), (5, 32, 32), (6, 32, 8), (7, 32, 32)],
    256: [(0, 64, 64), (1, 128, 64), (2, 128, 128), (3, 64, 64), (4, 64, 64), (5, 128, 128), (6, 64, 64), (7, 32, 32), (0, 128, 128)],
}
MAX_SIDE = {8: (8, 8), 16: (16, 16), 64: (32, 32), 256: (128, 128)}


def ref_off(l, x, y):
    return SLACK + l * PLANE + (MARGIN + y) * REF_STRIDE + MARGIN + x


def job_of(cfg, w, h, k, bd):
    x, y = (k * 24) % (PIC_W - w + 1) & ~3, (k * 40) % (PIC_H - h + 1) & ~3
    kw = dict(num_base=2, num_steps=8, dis_frac=0)
    B = mu.make_base
    if cfg == 0:      # equal distance on opposite sides: BDOF where the size allows it; a list-0 base
        bases = [B(mv=((6, -10), (-22, 13)), ref_idx=(0, 0), poc_diff=(-2, 2)), B(mv=((-9, 4), (0, 0)), ref_idx=(1, -1), poc_diff=(-4, 0))]
    elif cfg == 1:    # the scaled second offset on list 0 (list 1 is further away) and on list 1
        bases = [B(mv=((5, 3), (-18, 7)), ref_idx=(0, 0), poc_diff=(-1, 3)), B(mv=((-7, -12), (21, 2)), ref_idx=(1, 1), poc_diff=(4, -2))]
    elif cfg == 2:    # long-term: mirrored on opposite sides; a list-1 base
        bases = [B(mv=((2, 9), (-14, -3)), ref_idx=(0, 0), poc_diff=(-2, 5), long_term=(1, 0)), B(mv=((0, 0), (11, -6)), ref_idx=(-1, 0), poc_diff=(0, 3))]
    elif cfg == 3:    # BCW weights 10 and -2 (no BDOF under a weight)
        bases = [B(mv=((-3, 5), (12, -8)), ref_idx=(0, 0), poc_diff=(-2, 2), bcw=10), B(mv=((7, 7), (-2, 10)), ref_idx=(0, 1), poc_diff=(-1, -3), bcw=-2)]
    elif cfg == 4:    # the alternative half-sample filter: bases on the half-sample phase
        bases = [B(mv=((24, 8), (0, 0)), ref_idx=(0, -1), poc_diff=(-1, 0), alt_hpel=1), B(mv=((8, -8), (-24, 40)), ref_idx=(0, 1), poc_diff=(-1, 2), alt_hpel=1)]
    elif cfg == 5:    # whole-sample steps at a picture corner: clipMv engages
        x, y = PIC_W - w, PIC_H - h
        kw["dis_frac"] = 1
        hmax, vmax = (PIC_W + 8 - x - 1) << 4, (PIC_H + 8 - y - 1) << 4      # clipMv's upper limits here: the bases sit a few samples inside them
        bases = [B(mv=((hmax - 300, vmax - 200), (0, 0)), ref_idx=(0, -1), poc_diff=(-1, 0)), B(mv=((hmax - 100, 48), (-32, -16)), ref_idx=(0, 0), poc_diff=(-3, 3))]
    elif cfg == 6:    # a short loop: one base, three steps
        kw.update(num_base=1, num_steps=3)
        bases = [B(mv=((-5, 14), (9, -4)), ref_idx=(0, 0), poc_diff=(-2, 2)), B()]
    else:             # equal POC differences: one vector on both lists is predicted from list 0 alone; two vectors are averaged
        bases = [B(mv=((10, -6), (10, -6)), ref_idx=(0, 0), poc_diff=(-2, -2)), B(mv=((10, -6), (-13, 5)), ref_idx=(1, 1), poc_diff=(-2, -2), bcw=5)]
    for b in bases:
        b["ref_off"], b["ref_stride"] = [ref_off(0, x, y), ref_off(1, x, y)], [REF_STRIDE, REF_STRIDE]
    return mu.make_job(w, h, bases, pos=(x, y), bd=bd, bdof_allowed=1, org_off=y * PIC_W + x, org_stride=PIC_W, **kw)


@functools.lru_cache(maxsize=None)
def scene(bd):
    """original plane and the two reference planes (with their border) in one buffer; textured, so that every sample of motion shows in the cost"""
    rng = np.random.default_rng(100 + bd)
    yy, xx = np.mgrid[0:PIC_H + 2 * MARGIN, 0:REF_STRIDE]
    planes = []
    for l in range(2):
        smooth = ((np.sin(xx / (7.0 + l)) + np.cos(yy / (5.0 - l)) + 2.0) / 4.0 * ((1 << bd) - 1) * 0.6)
        noise = rng.integers(0, (1 << bd) * 4 // 10, smooth.shape)
        planes.append(np.clip(smooth + noise, 0, (1 << bd) - 1).astype(np.int16).reshape(-1))
    refs = np.ascontiguousarray(np.concatenate([np.zeros(SLACK, np.int16)] + planes + [np.zeros(SLACK, np.int16)]))
    org = np.ascontiguousarray(rng.integers(0, 1 << bd, (PIC_H, PIC_W)).astype(np.int16))
    return org, refs


def predict(L, refs, job, base, c, bd, bdof=None, bcw=None, alt=None, mv=None):
    """the luma prediction of candidate dict c; the keyword arguments replace what the candidate says (for the checks of the expectation)"""
    w, h = job["w"], job["h"]
    at = [C.c_void_p(refs.ctypes.data + 2 * base["ref_off"][l]) for l in range(2)]
    mv = c["pred_mv"] if mv is None else mv
    bdof = (c["kind"] == mu.BDOF) if bdof is None else bdof
    bcw = c["bcw"] if bcw is None else bcw
    alt = c["alt_hpel"] if alt is None else alt
    e = np.zeros((h, w), np.int16)
    if bdof:
        L.vo_bdof_pu(at[0], REF_STRIDE, at[1], REF_STRIDE, w, h, mv[0][0], mv[0][1], mv[1][0], mv[1][1], bd, ol.P(e), w)
    elif c["pred_mode"] == mu.PRED_BI:
        p = [np.zeros((h, w), np.int16) for _ in range(2)]
        for l in range(2):
            L.vo_mc_luma(at[l], REF_STRIDE, w, h, mv[l][0], mv[l][1], 1, bd, alt, ol.P(p[l]), w)
        if bcw == mu.BCW_DEFAULT:
            L.vo_add_avg(ol.P(p[0]), w, ol.P(p[1]), w, ol.P(e), w, w, h, bd)
        else:
            L.vo_add_weighted_avg(ol.P(p[0]), w, ol.P(p[1]), w, ol.P(e), w, w, h, bd, bcw)
    else:
        l = c["pred_mode"]
        L.vo_mc_luma(at[l], REF_STRIDE, w, h, mv[l][0], mv[l][1], 0, bd, alt, ol.P(e), w)
    return e


def costs_of(L, org, job, pred):
    po = C.c_void_p(org.ctypes.data + 2 * job["org_off"])
    return int(L.vo_satd(po, PIC_W, ol.P(pred), job["w"], job["w"], job["h"])), int(L.vo_sad(po, PIC_W, ol.P(pred), job["w"], job["w"], job["h"], 0))


@functools.lru_cache(maxsize=None)
def expectation(lanes, bd):
    """jobs, candidate dicts [job][64], costs [job][64][satd, sad] (NO_COST where not tested) -- computed once per batch and depth, shared and left unchanged"""
    L = ol.oracle()
    org, refs = scene(bd)
    jobs = [job_of(cfg, w, h, k, bd) for k, (cfg, w, h) in enumerate(BATCHES[lanes])]
    cands, costs = [], np.full((len(jobs), 64, 2), NO_COST, np.uint64)
    for i, job in enumerate(jobs):
        cs = mu.derive_all(job, (PIC_W, PIC_H, CTU))
        for c, d in enumerate(cs):
            if d["kind"] != mu.NOT_TESTED:
                costs[i, c] = costs_of(L, org, job, predict(L, refs, job, job["bases"][c // 32], d, bd))
        cands.append(cs)
    costs.setflags(write=False)
    return jobs, cands, costs


def check_expectation(lanes, bd):
    """the expectation depends on what the kernel must get right (CPU only)"""
    L = ol.oracle()
    org, refs = scene(bd)
    jobs, cands, costs = expectation(lanes, bd)
    pic = (PIC_W, PIC_H, CTU)
    seen = dict(scaled_l0=0, scaled_l1=0, mirror=0, alt=0, bcw10=0, bcw_2=0, clipped=0, bdof=0, bdof_differs=0, step3=0, short=0, identical=0)
    for i, (job, (cfg, w, h)) in enumerate(zip(jobs, BATCHES[lanes])):
        bi_allowed = w + h != 12
        for c, d in enumerate(cands[i]):
            if d["kind"] == mu.NOT_TESTED:
                continue
            base, step, pos = job["bases"][c // 32], (c % 32) // 4, c % 4
            d0, d1 = base["poc_diff"]
            cost = lambda **kw: costs_of(L, org, job, predict(L, refs, job, base, d, bd, **kw))      # noqa: E731
            mine = tuple(int(v) for v in costs[i, c])
            if d["inter_dir"] == 3 and d0 != d1 and (max(base["long_term"]) or abs(d0) != abs(d1)):
                # the unscaled offset: both lists move by the step
                off = mu.clip3(-(1 << 30), 1 << 30, ((1 << step) << 2) << (2 if job["dis_frac"] else 0)) * (-1 if pos & 1 else 1)
                other = 0 if abs(d1) > abs(d0) else 1
                mv = [list(d["mv"][0]), list(d["mv"][1])]
                mv[other] = [base["mv"][other][0] + (off if pos < 2 else 0), base["mv"][other][1] + (off if pos >= 2 else 0)]
                pmv = [mu.clip_mv(mv[l], (job["pos_x"], job["pos_y"]), pic[:2], CTU) for l in range(2)]
                if cost(mv=pmv) != mine:
                    seen["mirror" if max(base["long_term"]) else ("scaled_l0", "scaled_l1")[other]] += 1
            if d["kind"] == mu.BDOF:
                seen["bdof"] += 1
                seen["bdof_differs"] += cost(bdof=False) != mine
            if d["kind"] == mu.PLAIN and step == 3 and any(x["kind"] == mu.BDOF for x in cands[i][c - c % 32:c - c % 32 + 12]):
                seen["step3"] += cost(bdof=True) != mine
            if d["alt_hpel"] and any((v & 15) == 8 for l in range(2) for v in d["pred_mv"][l]):
                seen["alt"] += cost(alt=0) != mine
            if d["inter_dir"] == 3 and d["bcw"] in (10, -2):
                seen["bcw10" if d["bcw"] == 10 else "bcw_2"] += cost(bcw=mu.BCW_DEFAULT) != mine
            if cfg == 5:
                seen["clipped"] += d["pred_mv"] != d["mv"]
            seen["identical"] += d["inter_dir"] == 3 and d["pred_mode"] == mu.PRED_L0
        if cfg == 6:
            seen["short"] += sum(d["kind"] == mu.NOT_TESTED for d in cands[i]) == 64 - 12
        if cfg == 5:
            assert sum(d["pred_mv"] != d["mv"] for d in cands[i]) >= 4, (lanes, bd, i)
        if not bi_allowed:
            assert all(d["inter_dir"] != 3 for d in cands[i])
    for k in ("scaled_l0", "scaled_l1", "mirror", "alt", "bcw10", "bcw_2", "clipped", "short", "identical"):
        assert seen[k] > 0, (lanes, bd, seen)
    if MAX_SIDE[lanes][0] * MAX_SIDE[lanes][1] >= 128:
        assert seen["bdof"] > 0 and 2 * seen["bdof_differs"] >= seen["bdof"] and seen["step3"] > 0, (lanes, bd, seen)
    else:
        assert seen["bdof"] == 0
    return seen


def job_table(jobs):
    from vtm_amd.lib import MmvdJob
    arr = (MmvdJob * len(jobs))(*[mu.to_struct(j) for j in jobs])
    return np.frombuffer(arr, np.uint8).copy()


def run_device(ctx, lanes, bd, use_satd, jobs=None, expect_error=False):
    """-> (records [job][64] as tuples, costs [job * 64], guards intact)"""
    from vtm_amd.lib import MmvdCand, PicParams, VtmHipError
    org, refs = scene(bd)
    jobs = expectation(lanes, bd)[0] if jobs is None else jobs
    n = len(jobs)
    d_org, d_ref, d_jobs = ctx.to_device(org), ctx.to_device(refs), ctx.to_device(job_table(jobs))
    cand_bytes, dist_bytes = n * 64 * C.sizeof(MmvdCand), n * 64 * 8
    d_cand = ctx.to_device(np.full(cand_bytes + 2 * GUARD, 0xA5, np.uint8))
    d_dist = ctx.to_device(np.full(dist_bytes + 2 * GUARD, 0x5A, np.uint8))
    mw, mh = MAX_SIDE[lanes]
    try:
        err = None
        try:
            ctx.mmvd_cand_satd_batch(PicParams(PIC_W, PIC_H, CTU, bd), d_org.ptr, d_ref.ptr, d_jobs.ptr, n, mw, mh, d_cand.ptr + GUARD, d_dist.ptr + GUARD,
                                     use_satd=use_satd)
        except VtmHipError as e:
            err = e
        ctx.sync()
        raw_c, raw_d = d_cand.to_host(np.uint8), d_dist.to_host(np.uint8)
    finally:
        for b in (d_org, d_ref, d_jobs, d_cand, d_dist):
            b.free()
    guards = bool((raw_c[:GUARD] == 0xA5).all() and (raw_c[GUARD + cand_bytes:] == 0xA5).all() and (raw_d[:GUARD] == 0x5A).all() and (raw_d[GUARD + dist_bytes:] == 0x5A).all())
    if expect_error:
        return err, raw_c[GUARD:GUARD + cand_bytes], raw_d[GUARD:GUARD + dist_bytes], guards
    assert err is None, err
    recs = (MmvdCand * (n * 64)).from_buffer_copy(raw_c[GUARD:GUARD + cand_bytes].tobytes())
    return [mu.record_tuple(r) for r in recs], raw_d[GUARD:GUARD + dist_bytes].view(np.uint64).copy(), guards


def compare(lanes, bd, use_satd, recs, dist):
    jobs, cands, costs = expectation(lanes, bd)
    for i in range(len(jobs)):
        for c in range(64):
            assert recs[64 * i + c] == mu.record_tuple(cands[i][c]), (lanes, bd, BATCHES[lanes][i], c)
            assert int(dist[64 * i + c]) == int(costs[i, c, 0 if use_satd else 1]), (lanes, bd, use_satd, BATCHES[lanes][i], c, cands[i][c])
            if cands[i][c]["kind"] == mu.NOT_TESTED:
                assert int(dist[64 * i + c]) == NO_COST and recs[64 * i + c][9] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("lanes", [8, 16, 64, 256])
def test_mmvd_tables_match_the_expectation(ctx, lanes, bd):
    assert ctx.L.vtmhip_mc_lanes_per_block(*MAX_SIDE[lanes]) == lanes
    assert all(w <= MAX_SIDE[lanes][0] and h <= MAX_SIDE[lanes][1] for _, w, h in BATCHES[lanes])
    check_expectation(lanes, bd)
    for use_satd in (True, False):
        recs, dist, guards = run_device(ctx, lanes, bd, use_satd)
        assert guards, "a write outside d_cand / d_dist"
        compare(lanes, bd, use_satd, recs, dist)


def check_long_batches(ctx, lanes, sizes):
    jobs = expectation(lanes, 10)[0]
    recs, dist, guards = run_device(ctx, lanes, 10, True)
    compare(lanes, 10, True, recs, dist)
    err, base_c, base_d, guards = run_device(ctx, lanes, 10, True, expect_error=True)
    assert err is None and guards
    for n in sizes:
        err, raw_c, raw_d, guards = run_device(ctx, lanes, 10, True, jobs=(jobs * (n // len(jobs) + 1))[:n], expect_error=True)
        assert err is None and guards, n
        reps = n // len(jobs) + 1
        assert np.array_equal(raw_c, np.tile(base_c, reps)[:raw_c.size]) and np.array_equal(raw_d, np.tile(base_d, reps)[:raw_d.size]), (lanes, n)


@pytest.mark.gpu
@pytest.mark.parametrize("lanes,sizes", [(8, (517, 1034, 2057)), (16, (264, 517, 1034)), (64, (64, 128, 256)), (256, (64, 128, 256))])
def test_long_batches_take_the_other_candidates_per_item(ctx, lanes, sizes):
    """A lane group of the fused kernel walks 1, 2, 4 or 8 candidates of a CU, by the number of workgroups the batch gives (mmvd_fused_launch: 8 per CU of the device's
    256): the short batches above walk one each, these sizes two, four and eight.  The batch repeated must leave its tables repeated.  (The workgroup-sized batch
    takes the expansion here, with row counts in the thousands; its fused kernel sees these lengths in test_fused_route_on_workgroup_sized_blocks.)"""
    check_long_batches(ctx, lanes, sizes)


def test_batches_hold_the_shapes_the_kernel_can_go_wrong_at():
    shapes = {(w, h) for b in BATCHES.values() for _, w, h in b}
    assert {(8, 4), (4, 8), (8, 8), (16, 8), (8, 16), (16, 16), (32, 32), (64, 64), (128, 64), (128, 128)} <= shapes
    for lanes, b in BATCHES.items():
        assert {cfg for cfg, _, _ in b} == set(range(8))


def test_expectation_depends_on_what_the_kernel_must_get_right():
    """the same checks the GPU test makes before it asks the device, on the smallest batches (CPU only)"""
    check_expectation(8, 10)
    seen = check_expectation(16, 8)
    assert seen["bdof"] >= 24


@pytest.mark.gpu
def test_malformed_table_is_rejected_and_nothing_written(ctx):
    from vtm_amd import lib
    jobs = [dict(j, bases=[dict(b) for b in j["bases"]]) for j in expectation(16, 10)[0]]
    jobs[5]["num_steps"] = 9
    err, raw_c, raw_d, guards = run_device(ctx, 16, 10, True, jobs=jobs, expect_error=True)
    assert err is not None and err.status == lib.E_INVALID
    assert guards and (raw_c == 0xA5).all() and (raw_d == 0x5A).all()
    jobs[5]["num_steps"] = 8
    jobs[2]["w"] = 32      # above maxWidth
    err, raw_c, raw_d, guards = run_device(ctx, 16, 10, True, jobs=jobs, expect_error=True)
    assert err is not None and err.status == lib.E_INVALID and guards and (raw_c == 0xA5).all() and (raw_d == 0x5A).all()


def child_main(path, lanes):
    """one batch through whatever route the environment selects; the raw tables go to `path`.  The workgroup-sized batch also at the lengths that walk two, four and
    eight candidates per item (its default route is the expansion, so the parent's long batches never reach the fused kernel there)."""
    from vtm_amd.device import Context
    ctx = Context(0)
    out = {}
    for use_satd in (True, False):
        recs, dist, guards = run_device(ctx, lanes, 10, use_satd)
        assert guards
        out["recs%d" % use_satd], out["dist%d" % use_satd] = np.array(recs, np.int64), dist
    if lanes == 256:
        check_long_batches(ctx, lanes, (64, 128, 256))
    ctx.close()
    np.savez(path, **out)


def run_child(tmp_path, lanes, fused):
    path = str(tmp_path / "child.npz")
    env = dict(os.environ, VTMHIP_MMVD_FUSED=fused)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path, str(lanes)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    return np.load(path)


@pytest.mark.gpu
def test_expansion_route_leaves_identical_tables(ctx, tmp_path):
    """VTMHIP_MMVD_FUSED=0 (read once per process: a fresh child process) on the mixed batch, whose default route is the fused kernel"""
    z = run_child(tmp_path, 16, "0")
    for use_satd in (True, False):
        recs, dist, guards = run_device(ctx, 16, 10, use_satd)
        assert guards
        assert np.array_equal(np.array(recs, np.int64), z["recs%d" % use_satd]) and np.array_equal(dist, z["dist%d" % use_satd])
        compare(16, 10, use_satd, [tuple(int(v) for v in r) for r in z["recs%d" % use_satd]], z["dist%d" % use_satd])


@pytest.mark.gpu
def test_fused_route_on_workgroup_sized_blocks(ctx, tmp_path):
    """VTMHIP_MMVD_FUSED=1 on the batch of 64 x 64 .. 128 x 128 CUs, whose default route is the expansion: identical tables, and the expectation's"""
    z = run_child(tmp_path, 256, "1")
    for use_satd in (True, False):
        recs, dist, guards = run_device(ctx, 256, 10, use_satd)
        assert guards
        assert np.array_equal(np.array(recs, np.int64), z["recs%d" % use_satd]) and np.array_equal(dist, z["dist%d" % use_satd])
        compare(256, 10, use_satd, [tuple(int(v) for v in r) for r in z["recs%d" % use_satd]], z["dist%d" % use_satd])


if __name__ == "__main__":
    child_main(sys.argv[1], int(sys.argv[2]))
