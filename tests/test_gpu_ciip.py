"""GPU: vtmhip_ciip_cand_satd_batch_dev and vtmhip_ciip_blend_batch_dev against an expectation built without the library -- the inter blocks by the oracle
(vo_mc_luma, vo_add_avg), planar by intra_util (through ciip_util.planar), the LUTs and the blend in numpy, the costs by vo_satd / vo_sad.  Costs and kept blocks
must be bit-identical.

One batch per lane path of vtmhip_mc_lanes_per_block (8, 16, 64, 256 lanes) on the 256 x 192 scene of test_gpu_mmvd.py, 8-, 10- and 12-bit samples, SATD and SAD.
Before the device is asked, the expectation itself is shown to depend on what the kernel must get right (check_expectation): the line filter, PDPC, either LUT step,
the second list of a bi candidate, and the weight.  Malformed jobs are skipped on the device alone, a missing LUT fails the call, long batches repeat their tables,
and the call runs under a stream capture."""
import ctypes as C
import functools

import numpy as np
import pytest

import ciip_util as cu
import intra_util as iu
import oracle_lib as ol
import test_gpu_mmvd as tm      # the scene: original plane and two reference planes with their border

PIC_W, PIC_H, REF_STRIDE = tm.PIC_W, tm.PIC_H, tm.REF_STRIDE
NO_COST = cu.NO_COST
GUARD = 256      # bytes of pattern in front of and behind d_dist and the kept plane
DIST_FILL, KEEP_FILL = 0x5A, 0xA5

# (width, height) per job; what else a job carries comes from its index (job_of)
BATCHES = {
    8: [(8, 8)] * 10,
    16: [(16, 4), (4, 16), (16, 8), (16, 16), (8, 8), (8, 16), (16, 4), (4, 16), (16, 16), (16, 8)],
    64: [(32, 4), (32, 32), (4, 32), (16, 16), (32, 8), (32, 32), (8, 32), (32, 16), (16, 4), (32, 32)],
    256: [(64, 4), (4, 64), (64, 16), (64, 64), (32, 32), (16, 64), (64, 64), (64, 32), (8, 8), (64, 64)],
}
MAX_SIDE = {8: (8, 8), 16: (16, 16), 64: (32, 32), 256: (64, 64)}
MVS = [(6, -10), (-22, 13), (0, 0), (24, 8), (8, -8), (16, 32), (5, 3), (-18, 7), (40, 0), (0, -24)]      # fractional, whole-sample and half-sample phases, mixed


def job_of(k, w, h, bd):
    """job k of a batch: the weights, LMCS, the number of candidates, their modes, vectors, filter and kept flags all rotate with k"""
    x, y = (k * 24) % (PIC_W - w + 1) & ~3, (k * 40) % (PIC_H - h + 1) & ~3
    left, above = ((0, 0), (1, 0), (0, 1), (1, 1))[k % 4]
    cands = []
    for c in range((1, 3, 4)[k % 3]):
        mv = [MVS[(3 * k + 2 * c + l) % len(MVS)] for l in range(2)]
        alt = int((k + c) % 3 == 0 or any((v & 15) == 8 for m in mv for v in m) and c % 2 == 0)
        cands.append(cu.make_cand(mode=(k + c) % 4, ref_off=(tm.ref_off(0, x, y), tm.ref_off(1, x, y)), ref_stride=(REF_STRIDE, REF_STRIDE), mv=mv, alt=alt,
                                  src_stride=w + 4, keep_off=0 if (k + c) % 2 == 0 else -1))
    return cu.make_job(w, h, bd, cands, left=left, above=above, lmcs=(k // 2) % 2, org_off=y * PIC_W + x, org_stride=PIC_W)


def inter_block(L, refs, w, h, c, bd, drop_second=False):
    """the plain inter luma block of a candidate; a given block (mode 3) holds the list-0 prediction of its vector"""
    at = [C.c_void_p(refs.ctypes.data + 2 * c["ref_off"][l]) for l in range(2)]
    e = np.zeros((h, w), np.int16)
    if c["mode"] == cu.BI and not drop_second:
        p = [np.zeros((h, w), np.int16) for _ in range(2)]
        for l in range(2):
            L.vo_mc_luma(at[l], REF_STRIDE, w, h, c["mv"][l][0], c["mv"][l][1], 1, bd, c["alt"], ol.P(p[l]), w)
        L.vo_add_avg(ol.P(p[0]), w, ol.P(p[1]), w, ol.P(e), w, w, h, bd)
    else:
        l = 1 if c["mode"] == cu.L1 else 0
        L.vo_mc_luma(at[l], REF_STRIDE, w, h, c["mv"][l][0], c["mv"][l][1], 0, bd, c["alt"], ol.P(e), w)
    return e


def costs_of(L, org, job, seen):
    po, seen = C.c_void_p(org.ctypes.data + 2 * job["org_off"]), np.ascontiguousarray(seen)
    return int(L.vo_satd(po, PIC_W, ol.P(seen), job["w"], job["w"], job["h"])), int(L.vo_sad(po, PIC_W, ol.P(seen), job["w"], job["w"], job["h"], 0))


class Batch:
    """jobs with their lines, given blocks and kept slots laid out, and what the device must leave: costs [job][4][satd, sad] and the kept plane"""

    def __init__(self, shapes, bd, jobs=None):
        L, rng = ol.oracle(), np.random.default_rng(1000 + bd + len(shapes) + shapes[0][0])
        self.bd, self.org, self.refs = bd, *tm.scene(bd)
        self.fwd, self.inv = cu.make_luts(bd)
        self.jobs = [job_of(k, w, h, bd) for k, (w, h) in enumerate(shapes)] if jobs is None else jobs
        lines, given, kept = [np.zeros(3, np.int16)], [np.zeros(5, np.int16)], 0      # odd first offsets: nothing is aligned beyond a sample
        line_at, given_at = 3, 5
        self.lines_of, self.inters = [], []
        for job in self.jobs:
            w, h = job["w"], job["h"]
            wl, hl = (w, h) if cu.size_ok(w, h) else (8, 8)      # a malformed size: no lines are read through it
            ln = np.concatenate(iu.make_lines(rng, wl, hl, 0, bd, "random"))
            job["line_off"] = line_at
            lines.append(ln)
            line_at += ln.size
            self.lines_of.append(ln)
            blocks = []
            for c in job["cands"]:
                e = inter_block(L, self.refs, wl, hl, c, bd) if c["mode"] <= cu.GIVEN else np.zeros((hl, wl), np.int16)
                blocks.append(e)
                if c["mode"] >= cu.GIVEN:
                    stride = c["src_stride"]
                    pool = rng.integers(0, 1 << bd, (hl, max(stride, wl))).astype(np.int16)
                    pool[:, :wl] = e
                    c["src_off"] = given_at
                    given.append(pool.reshape(-1))
                    given_at += pool.size
                if c["keep_off"] >= 0:
                    c["keep_off"] = kept      # relative to the kept plane; device_tables adds the plane's position
                kept += wl * hl
            self.inters.append(blocks)
        self.lines, self.given, self.kept_samples = np.concatenate(lines), np.concatenate(given), kept
        self.costs = np.full((len(self.jobs), 4, 2), NO_COST, np.uint64)
        self.kept = np.full(kept, KEEP_FILL * 0x0101, np.uint16).view(np.int16)

    def expect(self, ok=None):
        """fills costs and the kept plane; ok[i] == False: job i is malformed and must be skipped"""
        L = ol.oracle()
        for i, job in enumerate(self.jobs):
            if ok is not None and not ok[i]:
                continue
            intra = cu.planar(self.lines_of[i][:2 * job["w"] + 1], self.lines_of[i][2 * job["w"] + 1:], job["w"], job["h"])
            wi = cu.weight_intra(job["left"], job["above"])
            for k, c in enumerate(job["cands"]):
                mapped, seen = cu.candidate(self.inters[i][k], intra, wi, self.fwd if job["lmcs"] else None, self.inv if job["lmcs"] else None)
                self.costs[i, k] = costs_of(L, self.org, job, seen)
                if c["keep_off"] >= 0:
                    self.kept[c["keep_off"]:c["keep_off"] + mapped.size] = mapped.reshape(-1)
        self.costs.setflags(write=False)
        self.kept.setflags(write=False)
        return self


@functools.lru_cache(maxsize=None)
def expectation(lanes, bd):
    """computed once per (path, depth), shared and left unchanged"""
    return Batch(BATCHES[lanes], bd).expect()


def check_expectation(lanes, bd):
    """the expectation depends on what the kernel must get right (CPU only): every probe changes at least one cost of the batch"""
    L = ol.oracle()
    b = expectation(lanes, bd)
    seen = dict(filter=0, pdpc=0, fwd=0, inv=0, second=0, weight_up=0, weight_down=0, alt_half=0, kept=0, given=0)
    for i, job in enumerate(b.jobs):
        w, h, ln = job["w"], job["h"], b.lines_of[i]
        top, left = ln[:2 * w + 1], ln[2 * w + 1:]
        intra, wi = cu.planar(top, left, w, h), cu.weight_intra(job["left"], job["above"])
        fwd, inv = (b.fwd, b.inv) if job["lmcs"] else (None, None)
        for k, c in enumerate(job["cands"]):
            mine = tuple(int(v) for v in b.costs[i, k])
            cost = lambda inter=b.inters[i][k], intra=intra, wi=wi, fwd=fwd, inv=inv: costs_of(L, b.org, job, cu.candidate(inter, intra, wi, fwd, inv)[1])      # noqa: E731
            assert cost() == mine
            seen["filter"] += cost(intra=cu.planar(top, left, w, h, filt=False)) != mine
            seen["pdpc"] += cost(intra=cu.planar(top, left, w, h, pdpc=False)) != mine
            if job["lmcs"]:
                seen["fwd"] += cost(fwd=None) != mine
                seen["inv"] += cost(inv=None) != mine
            if c["mode"] == cu.BI:
                seen["second"] += cost(inter=inter_block(L, b.refs, w, h, c, bd, drop_second=True)) != mine
            seen["weight_up"] += cost(wi=wi % 3 + 1) != mine
            seen["weight_down"] += cost(wi=(wi + 1) % 3 + 1) != mine
            if c["alt"] and c["mode"] != cu.GIVEN:
                lists = (0, 1) if c["mode"] == cu.BI else (c["mode"],)
                if any((v & 15) == 8 for l in lists for v in c["mv"][l]):
                    seen["alt_half"] += cost(inter=inter_block(L, b.refs, w, h, dict(c, alt=0), bd)) != mine
            seen["kept"] += c["keep_off"] >= 0
            seen["given"] += c["mode"] == cu.GIVEN
    assert all(v > 0 for v in seen.values()), (lanes, bd, seen)
    assert {j["num_cand"] for j in b.jobs} == {1, 3, 4} and {cu.weight_intra(j["left"], j["above"]) for j in b.jobs} == {1, 2, 3}
    assert {j["lmcs"] for j in b.jobs} == {0, 1} and {c["mode"] for j in b.jobs for c in j["cands"]} == {0, 1, 2, 3}
    assert any(c["keep_off"] < 0 for j in b.jobs for c in j["cands"])
    return seen


def device_tables(b, reps=1):
    """-> (job table bytes, the d_pred image: given pool | guard | kept plane x reps | guard, the kept plane's first sample)"""
    from vtm_amd.lib import CiipJob
    keep_at = b.given.size + GUARD // 2
    structs = []
    for r in range(reps):
        for job in b.jobs:
            s = cu.to_struct(job)
            for k in range(min(4, len(job["cands"]))):
                if job["cands"][k]["keep_off"] >= 0:
                    s.cand[k].keepOff = keep_at + r * b.kept_samples + job["cands"][k]["keep_off"]
            structs.append(s)
    table = np.frombuffer((CiipJob * len(structs))(*structs), np.uint8).copy()
    pred = np.concatenate([b.given, np.full(GUARD // 2 + reps * b.kept_samples + GUARD // 2, KEEP_FILL * 0x0101, np.uint16).view(np.int16)])
    return table, pred, keep_at


def run_device(ctx, b, lanes, use_satd, reps=1, call_lmcs=True, n=None, launch=None):
    """-> (error, costs [n * 4], the kept plane's samples, guards intact)"""
    from vtm_amd.lib import VtmHipError
    table, pred, keep_at = device_tables(b, reps)
    n = reps * len(b.jobs) if n is None else n
    if call_lmcs:
        ctx.set_lmcs_fwd_lut(b.fwd, b.bd)
        ctx.set_lmcs_inv_lut(b.inv, b.bd)
    d_ref, d_line, d_org, d_pred, d_jobs = (ctx.to_device(a) for a in (b.refs, b.lines, b.org, pred, table))
    d_dist = ctx.to_device(np.full(n * 32 + 2 * GUARD, DIST_FILL, np.uint8))
    mw, mh = MAX_SIDE[lanes]
    try:
        err = None
        try:
            call = lambda: ctx.ciip_cand_satd_batch(d_ref.ptr, d_line.ptr, d_org.ptr, d_pred.ptr, d_jobs.ptr, n, mw, mh, d_dist.ptr + GUARD, use_satd=use_satd,      # noqa: E731
                                                    lmcs=call_lmcs)
            call() if launch is None else launch(call)
        except VtmHipError as e:
            err = e
        ctx.sync()
        raw_d, raw_p = d_dist.to_host(np.uint8), d_pred.to_host(np.int16)
    finally:
        for buf in (d_ref, d_line, d_org, d_pred, d_jobs, d_dist):
            buf.free()
    fill = np.int16(np.uint16(KEEP_FILL * 0x0101).view(np.int16))
    guards = bool((raw_d[:GUARD] == DIST_FILL).all() and (raw_d[GUARD + n * 32:] == DIST_FILL).all() and (raw_p[b.given.size:keep_at] == fill).all() and
                  (raw_p[keep_at + reps * b.kept_samples:] == fill).all() and np.array_equal(raw_p[:b.given.size], b.given))
    return err, raw_d[GUARD:GUARD + n * 32].view(np.uint64).copy(), raw_p[keep_at:keep_at + reps * b.kept_samples].copy(), guards


def compare(b, use_satd, dist, kept, where):
    for i, job in enumerate(b.jobs):
        for k in range(4):
            assert int(dist[4 * i + k]) == int(b.costs[i, k, 0 if use_satd else 1]), (where, use_satd, i, (job["w"], job["h"]), k, job["cands"][k] if k < len(job["cands"]) else None)
    assert np.array_equal(kept, b.kept), where      # kept blocks exact, unkept slots still the pattern


@pytest.mark.gpu
@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("lanes", [8, 16, 64, 256])
def test_ciip_costs_and_kept_blocks_match_the_expectation(ctx, lanes, bd):
    assert ctx.L.vtmhip_mc_lanes_per_block(*MAX_SIDE[lanes]) == lanes
    check_expectation(lanes, bd)
    b = expectation(lanes, bd)
    for use_satd in (True, False):
        err, dist, kept, guards = run_device(ctx, b, lanes, use_satd)
        assert err is None, err
        assert guards, "a write outside d_dist / the kept plane"
        compare(b, use_satd, dist, kept, (lanes, bd))


def test_batches_hold_the_shapes_the_kernel_can_go_wrong_at():
    shapes = {s for b in BATCHES.values() for s in b}
    assert {(8, 8), (16, 4), (4, 16), (16, 8), (16, 16), (32, 4), (32, 32), (64, 4), (4, 64), (64, 16), (64, 64)} <= shapes
    for lanes, b in BATCHES.items():
        assert all(w <= MAX_SIDE[lanes][0] and h <= MAX_SIDE[lanes][1] and cu.size_ok(w, h) for w, h in b)
        assert max(w * h for w, h in b) == MAX_SIDE[lanes][0] * MAX_SIDE[lanes][1]


def test_expectation_depends_on_what_the_kernel_must_get_right():
    """the same checks the GPU test makes before it asks the device, on the two smallest batches (CPU only)"""
    check_expectation(8, 10)
    check_expectation(16, 8)


def malformed_batch(bd):
    """the 16-lane batch for a call with lmcs = 0: no job asks for LMCS but job 9, and jobs 1, 3, 4, 7 are broken one field each"""
    jobs = [job_of(k, w, h, bd) for k, (w, h) in enumerate(BATCHES[16])]
    for j in jobs:
        j["lmcs"] = 0
    jobs[1]["w"], jobs[1]["h"] = 4, 8
    jobs[3]["w"] = 128
    jobs[4]["num_cand"] = 5
    jobs[7]["cands"][1]["mode"] = 4
    jobs[9]["lmcs"] = 1
    ok = [i not in (1, 3, 4, 7, 9) for i in range(len(jobs))]
    return Batch(BATCHES[16], bd, jobs=jobs).expect(ok), ok


@pytest.mark.gpu
def test_malformed_jobs_are_skipped_alone(ctx):
    b, ok = malformed_batch(10)
    assert sum(ok) == 5 and b.jobs[4]["cands"][0]["keep_off"] >= 0 and b.jobs[7]["cands"][1]["keep_off"] >= 0      # skipped jobs that asked for a kept block
    for use_satd in (True, False):
        err, dist, kept, guards = run_device(ctx, b, 16, use_satd, call_lmcs=False)
        assert err is None and guards
        compare(b, use_satd, dist, kept, "malformed")
        for i, good in enumerate(ok):
            if not good:
                assert [int(v) for v in dist[4 * i:4 * i + 4]] == [NO_COST] * 4


@pytest.mark.gpu
def test_lmcs_without_the_inverse_lut_fails_before_anything_runs():
    from vtm_amd import lib
    from vtm_amd.device import Context
    b = expectation(16, 10)
    own = Context(0)
    try:
        for step in range(3):      # no LUT at all; the forward LUT alone; both, of different depths
            if step == 1:
                own.set_lmcs_fwd_lut(b.fwd, 10)
            if step == 2:
                own.set_lmcs_inv_lut(cu.make_luts(8)[1], 8)
            table, pred, keep_at = device_tables(b)
            d = [own.to_device(a) for a in (b.refs, b.lines, b.org, pred, table, np.full(len(b.jobs) * 32, DIST_FILL, np.uint8))]
            with pytest.raises(lib.VtmHipError) as e:
                own.ciip_cand_satd_batch(d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr, d[4].ptr, len(b.jobs), 16, 16, d[5].ptr, lmcs=True)
            assert e.value.status == lib.E_INVALID
            own.sync()
            assert (d[5].to_host(np.uint8) == DIST_FILL).all() and np.array_equal(d[3].to_host(np.int16), pred)
            for buf in d:
                buf.free()
    finally:
        own.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lanes,reps,n", [(8, 8, 77), (16, 5, 43), (64, 3, 25), (256, 3, 21)])
def test_long_batches_repeat_their_tables(ctx, lanes, reps, n):
    """the batch repeated: a workgroup of the 8- and 16-lane paths holds eight and four CUs, and n leaves the last one partly empty"""
    b = expectation(lanes, 10)
    err, base_d, base_k, guards = run_device(ctx, b, lanes, True)
    assert err is None and guards
    compare(b, True, base_d, base_k, lanes)
    err, dist, kept, guards = run_device(ctx, b, lanes, True, reps=reps, n=n)
    assert err is None and guards
    assert lanes >= 64 or n % {8: 8, 16: 4}[lanes] != 0
    assert np.array_equal(dist, np.tile(base_d, reps)[:dist.size]), lanes
    done = n // len(b.jobs)      # whole repetitions; the jobs of the cut one leave their kept blocks, the others the pattern
    assert np.array_equal(kept[:done * b.kept_samples], np.tile(base_k, done))
    fill = np.uint16(KEEP_FILL * 0x0101).view(np.int16)
    tail = np.full(b.kept_samples, fill, np.int16)
    for job in b.jobs[:n - done * len(b.jobs)]:
        for c in job["cands"]:
            if c["keep_off"] >= 0:
                tail[c["keep_off"]:c["keep_off"] + job["w"] * job["h"]] = b.kept[c["keep_off"]:c["keep_off"] + job["w"] * job["h"]]
    assert np.array_equal(kept[done * b.kept_samples:(done + 1) * b.kept_samples], tail)
    assert (kept[(done + 1) * b.kept_samples:] == fill).all()


def hip_runtime():
    """the HIP runtime this process has mapped already (the one libvtmhip.so is bound to), by its path: a second copy would own no device"""
    with open("/proc/self/maps") as f:
        paths = {line.split()[-1] for line in f if "libamdhip64.so" in line}
    assert len(paths) == 1, paths
    return C.CDLL(paths.pop())


@pytest.mark.gpu
def test_call_runs_under_a_stream_capture_and_replays():
    """captured on the context's stream in the strictest capture mode (one branch: a single launch), replayed once: the tables of the eager call"""
    from vtm_amd.device import Context
    b = expectation(16, 10)
    own = Context(0)
    H = hip_runtime()
    stream, graph, graph_exec = C.c_void_p(), C.c_void_p(), C.c_void_p()
    try:
        err, eager_d, eager_k, guards = run_device(own, b, 16, True)
        assert err is None and guards
        compare(b, True, eager_d, eager_k, "eager")
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

        err, dist, kept, guards = run_device(own, b, 16, True, launch=launch)
        assert err is None and guards
        assert np.array_equal(dist, eager_d) and np.array_equal(kept, eager_k)
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
BLEND_TABLES = {      # (width, height, chroma, mapFwd) per job; lanes per job by the largest well-formed block
    16: [(4, 4, 1, 0), (8, 8, 0, 0), (8, 4, 1, 0), (2, 8, 1, 0), (8, 2, 1, 0), (16, 4, 0, 1), (4, 4, 1, 0), (4, 16, 0, 0), (8, 8, 0, 1)] * 2 + [(4, 4, 1, 0)],
    64: [(4, 16, 1, 0), (32, 32, 1, 0), (16, 16, 0, 1), (2, 16, 1, 0), (32, 8, 0, 0), (8, 4, 1, 0), (32, 32, 0, 0), (16, 2, 1, 0), (8, 8, 0, 0), (4, 4, 1, 0), (32, 32, 1, 0)],
    256: [(64, 64, 0, 1), (32, 32, 1, 0), (4, 4, 1, 0), (64, 16, 0, 0), (2, 32, 1, 0), (4, 64, 0, 0), (64, 64, 0, 0)],
}


@functools.lru_cache(maxsize=None)
def blend_case(lanes, bd):
    """-> (job table bytes, lines, the plane before, the plane after): every block sits inside a rim of pattern, a width-2 block stays as it is"""
    from vtm_amd.lib import CiipBlendJob
    import intra_util as iu
    rng = np.random.default_rng(50 + lanes + bd)
    fwd, _ = cu.make_luts(bd)
    structs, lines, before, after, line_at, at = [], [np.zeros(1, np.int16)], [], [], 1, 0
    for k, (w, h, chroma, map_fwd) in enumerate(BLEND_TABLES[lanes]):
        left, above = ((1, 1), (0, 0), (1, 0), (0, 1))[k % 4]
        ln = np.concatenate(iu.make_lines(rng, w, h, 0, bd, "random"))
        stride = w + (k % 3) * 3
        plane = rng.integers(0, 1 << bd, (h + 2, stride + 4)).astype(np.int16)
        inter = plane[1:-1, 2:2 + w].copy()
        out = plane.copy()
        if w > 2:
            intra = cu.planar(ln[:2 * w + 1], ln[2 * w + 1:], w, h, filt=not chroma)
            out[1:-1, 2:2 + w] = cu.blend(cu.lut(fwd, inter) if map_fwd else inter, intra, cu.weight_intra(left, above))
        structs.append(cu.blend_struct(w, h, bd, line_at, at + plane.shape[1] + 2, plane.shape[1], chroma=chroma, left=left, above=above, map_fwd=map_fwd))
        lines.append(ln); before.append(plane.reshape(-1)); after.append(out.reshape(-1))      # noqa: E702
        line_at += ln.size
        at += plane.size
    table = np.frombuffer((CiipBlendJob * len(structs))(*structs), np.uint8).copy()
    return table, np.concatenate(lines), np.concatenate(before), np.concatenate(after), fwd


@pytest.mark.gpu
@pytest.mark.parametrize("bd", [8, 10, 12])
@pytest.mark.parametrize("lanes", [16, 64, 256])
def test_blend_entry_in_place_against_numpy(ctx, lanes, bd):
    table, lines, before, after, fwd = blend_case(lanes, bd)
    n = len(BLEND_TABLES[lanes])
    assert ctx.L.vtmhip_intra_lanes_per_job(max(w * h for w, h, _, _ in BLEND_TABLES[lanes] if w > 2)) == lanes
    assert not np.array_equal(before, after)
    ctx.set_lmcs_fwd_lut(fwd, bd)
    d_line, d_pred, d_jobs = ctx.to_device(lines), ctx.to_device(before), ctx.to_device(table)
    try:
        ctx.ciip_blend_batch(d_line.ptr, d_pred.ptr, d_jobs.ptr, n)
        ctx.sync()
        got = d_pred.to_host(np.int16)
    finally:
        for buf in (d_line, d_pred, d_jobs):
            buf.free()
    assert np.array_equal(got, after), (lanes, bd, np.flatnonzero(got != after)[:8])


def test_blend_tables_hold_the_issue_shapes():
    chroma = {(w, h) for t in BLEND_TABLES.values() for w, h, c, _ in t if c}
    assert {(4, 4), (8, 4), (4, 16), (32, 32)} <= chroma and any(w == 2 for w, _ in chroma)
    for t in BLEND_TABLES.values():
        assert {c for _, _, c, _ in t} == {0, 1} and any(m for _, _, _, m in t)


@pytest.mark.gpu
def test_blend_map_fwd_without_a_lut_of_the_depth_is_skipped():
    """a fresh context has no forward LUT: the mapFwd jobs alone stay as they are"""
    from vtm_amd.device import Context
    table, lines, before, after, fwd = blend_case(16, 10)
    own = Context(0)
    try:
        d_line, d_pred, d_jobs = own.to_device(lines), own.to_device(before), own.to_device(table)
        own.ciip_blend_batch(d_line.ptr, d_pred.ptr, d_jobs.ptr, len(BLEND_TABLES[16]))
        own.sync()
        got = d_pred.to_host(np.int16)
    finally:
        own.close()
    at, want = 0, after.copy()
    for k, (w, h, chroma, map_fwd) in enumerate(BLEND_TABLES[16]):
        size = (h + 2) * (w + (k % 3) * 3 + 4)
        if map_fwd:
            want[at:at + size] = before[at:at + size]
        at += size
    assert np.array_equal(got, want)
