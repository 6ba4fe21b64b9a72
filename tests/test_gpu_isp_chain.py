"""GPU: vtmhip_isp_chain_batch_dev on every lane path against vtmhip_isp_chain_host (pinned by tests/test_isp.py) in full -- every buffer, the fill between the
blocks included -- and, for the CUs up to 16x16, against the composition of isp_util (the restatement and the oracle), which rests on no entry of the library.

The paths: 16 lanes per job (CUs up to 64 samples), 64 lanes (up to 1024 samples), 256 lanes (above, and wherever a 64-point transform makes four jobs too large for
the workgroup's LDS: 4x64, 64x4, 64x16, 16x64 -- the first two would have a wave by their area; they are tested on the path the entry gives them).  The 256-lane
table also holds a 16x16 and an 8x4 CU, which take that path with the table, so that it too is checked against the composition.
Before the device is asked, the expectation alone is shown to depend on what the kernel must get right:
  1. at least half of the jobs of a path have absSum > 0 in a sub-partition that is not the last, so later predictions see a reconstruction that is not the prediction;
  2. for at least half of the jobs the assembled prediction differs from the one formed from the original in place of the reconstruction, and from the prediction of
     the whole CU without ISP;
  3. the clip case (originals within 3 of either end of the range, base QP 44 .. 53) clips at both ends and separates sse from the residual-domain SSE;
  4. a job per path has a sub-partition with absSum == 0 between two with absSum > 0 (its original there is its own prediction)."""
import ctypes as C

import numpy as np
import pytest

import intra_util as iu
import isp_util as isp
from vtm_amd import lib
from vtm_amd.lib import DistJob

pytestmark = pytest.mark.gpu

MODES = [0, 1, 2, 18, 34, 50, 66, 7, 61, 45, 23, 56]
QPS = [12, 27, 37, 51]
PATHS = {
    16: [(4, 8), (8, 4), (4, 16), (16, 4), (8, 8)],
    64: [(8, 16), (16, 8), (16, 16), (32, 8), (8, 32)],
    256: [(32, 32), (64, 64), (64, 16), (16, 64), (4, 64), (64, 4), (16, 16), (8, 4)],          # the lane form follows the largest CU: the small ones ride on it
}
GAP_SHAPE = {16: (8, 8), 64: (16, 16), 256: (32, 32)}
_cache = {}


def _jobs_of(per_block):
    def f(i, b):
        out = []
        for k in range(per_block):
            split = 1 + (k & 1)
            out.append((MODES[(3 * i + k) % len(MODES)], split, (k >> 1) & 1, QPS[(i + (k >> 1)) % 4], (i + k) & 1))
        return out
    return f


def _gap_job(batch, k):
    """make sub-partition 1 of job k (the only job of its block) quantise to nothing: its original becomes its own prediction, which depends on sub-partition 0 only"""
    i = batch.jobs[k][0]
    b, j = batch.blocks[i], batch.job_arr[k]
    g = isp.geometry(b["w"], b["h"], batch.jobs[k][2])
    assert g["numParts"] == 4
    pred = batch.host()["pred"][j.predOff:j.predOff + b["w"] * b["h"]].reshape(b["h"], b["w"])
    x, y = b["org_xy"]
    px, py = (0, g["partH"]) if batch.jobs[k][2] == isp.HOR else (g["partW"], 0)
    batch.plane[y + py:y + py + g["partH"], x + px:x + px + g["partW"]] = pred[py:py + g["partH"], px:px + g["partW"]]
    batch._host = None


def path_batch(lanes):
    if lanes not in _cache:
        rng = np.random.default_rng(100 + lanes)
        shapes = [(w, h, (8, 10, 12)[(i + lanes) % 3]) for i, (w, h) in enumerate(PATHS[lanes])]
        gw, gh = GAP_SHAPE[lanes]
        shapes += [(gw, gh, 10), (gw, gh, 10)]          # the two gap jobs (one per split) have blocks of their own
        per = 8 if lanes == 16 else 4

        def jobs_of(i, b):
            if i >= len(PATHS[lanes]):
                return [(1, 1 + (i - len(PATHS[lanes])), 1, 30, 0)]
            return _jobs_of(per)(i, b)
        n = len(PATHS[lanes]) * per + 2
        order = list(np.random.default_rng(7).permutation(n))     # a shuffled table
        b = isp.make_batch(rng, shapes, jobs_of, order=order)
        for k, j in enumerate(b.jobs):
            if j[0] >= len(PATHS[lanes]):
                _gap_job(b, k)
        got = C.c_int()
        assert lib.load().vtmhip_isp_chain_lanes_host(C.addressof(b.blk_arr), len(b.blocks), C.addressof(b.job_arr), b.n, C.byref(got)) == lib.OK
        assert got.value == lanes
        assert b.n % (256 // lanes) != 0 or lanes == 256          # the last workgroup is partly filled
        _cache[lanes] = b
    return _cache[lanes]


@pytest.fixture(scope="module")
def ctx():
    from vtm_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _conditions(b):
    """conditions 1, 2 and 4 on the expectation of a path"""
    res = b.host()["results"]
    nonlast = sum(any(int(r["absSum"][p]) > 0 for p in range(int(r["numParts"]) - 1)) for r in res[:b.n])
    assert 2 * nonlast >= b.n, (nonlast, b.n)
    assert any(int(r["numParts"]) == 4 and int(r["absSum"][0]) > 0 and int(r["absSum"][1]) == 0 and int(r["absSum"][2]) > 0 for r in res[:b.n])
    differs = 0
    for k, (i, mode, split, avail, qp, irap) in enumerate(b.jobs):
        blk, j = b.blocks[i], b.job_arr[k]
        pred = b.host()["pred"][j.predOff:j.predOff + blk["w"] * blk["h"]].reshape(blk["h"], blk["w"])
        whole = iu.predict(blk["top"], blk["left"], blk["w"], blk["h"], mode, 0, blk["bd"], [])
        differs += int(not np.array_equal(pred, b.composed(k, from_org=True)["pred"]) and not np.array_equal(pred, whole))
    assert 2 * differs >= b.n, (differs, b.n)


@pytest.mark.parametrize("lanes", [16, 64, 256])
def test_isp_chain_path(ctx, lanes):
    b = path_batch(lanes)
    _conditions(b)
    st, got = b.run_dev(ctx)
    assert st == lib.OK
    isp.Batch.same(got, b.host())
    composed = 0
    for k, j in enumerate(b.jobs):                    # ... and without any entry of the library, up to 16x16
        if b.blocks[j[0]]["w"] <= 16 and b.blocks[j[0]]["h"] <= 16:
            b.check_composed(got, k)
            composed += 1
    assert composed >= 4, composed                    # every lane path rests on the composition for some of its jobs


@pytest.mark.parametrize("lanes", [16, 64, 256])
def test_isp_chain_optional_outputs_and_prefix(ctx, lanes):
    b = path_batch(lanes)
    st, got = b.run_dev(ctx, pred=False, levels=False)
    assert st == lib.OK
    isp.Batch.same(got, b.host(), pred=False, levels=False)
    n = b.n - 3                                        # a shorter table: the jobs past it stay fill
    st, got = b.run_dev(ctx, n=n)
    st2, exp = b.run_host(n=n)
    assert st == lib.OK and st2 == lib.OK
    isp.Batch.same(got, exp)
    assert (got["results"][n:].view(np.uint8) == isp.FILL).all()
    st, got = b.run_dev(ctx, n=0)
    assert st == lib.OK and isp.Batch.untouched(got)


def test_isp_chain_clip_case(ctx):
    """originals within 3 of either end of the range, base QP 44 .. 53: the reconstruction clips at both ends"""
    rng = np.random.default_rng(11)

    def org(rng, b):
        mx = (1 << b["bd"]) - 1
        lo = rng.integers(0, 2, (b["h"], b["w"]))
        return np.where(lo, rng.integers(0, 4, (b["h"], b["w"])), mx - rng.integers(0, 4, (b["h"], b["w"])))
    shapes = [(8, 8, 8), (16, 16, 10), (16, 4, 12), (32, 32, 10)]
    b = isp.make_batch(rng, shapes, lambda i, blk: [(MODES[(i + k) % 7], 1 + (k & 1), k >> 1 & 1, 44 + (3 * i + 5 * k) % 10, k & 1) for k in range(4)], org=org)
    clipped, separate = [0, 0], 0
    for k in range(b.n):
        if b.blocks[b.jobs[k][0]]["w"] <= 16:
            e = b.composed(k)
            clipped = [clipped[0] + e["clipped"][0], clipped[1] + e["clipped"][1]]
            separate += int(e["sse"] != e["sseResi"])
    assert clipped[0] > 0 and clipped[1] > 0 and separate > 0, (clipped, separate)
    st, got = b.run_dev(ctx)
    assert st == lib.OK
    isp.Batch.same(got, b.host())
    for k in range(b.n):
        if b.blocks[b.jobs[k][0]]["w"] <= 16:
            b.check_composed(got, k)


def test_isp_chain_sse_is_the_distortion_entry(ctx):
    """sse[k] == vtmhip_dist_batch_dev( VTMHIP_DIST_SSE ) of the original against the output on the rectangle of sub-partition k"""
    from vtm_amd.device import struct_array_to_numpy as s2n
    b = path_batch(64)
    st, got = b.run_dev(ctx)
    assert st == lib.OK
    items = []
    for k, (i, mode, split, avail, qp, irap) in enumerate(b.jobs):
        blk, j = b.blocks[i], b.job_arr[k]
        g = isp.geometry(blk["w"], blk["h"], split)
        for p in range(g["numParts"]):
            px, py = (0, p * g["partH"]) if split == isp.HOR else (p * g["partW"], 0)
            items.append((k, p, DistJob(blk["org_off"] + py * blk["org_stride"] + px, j.outOff + py * blk["w"] + px, blk["org_stride"], blk["w"], g["partW"], g["partH"], 0,
                                        lib.DIST_SSE)))
    arr = (DistJob * len(items))(*[it[2] for it in items])
    d_org, d_cur, d_dj, d_out = ctx.to_device(np.ascontiguousarray(b.plane)), ctx.to_device(got["reco"]), ctx.to_device(s2n(arr)), ctx.alloc(8 * len(items))
    ctx.dist_batch(d_org.ptr, d_cur.ptr, d_dj.ptr, len(items), d_out.ptr)
    ctx.sync()
    out = d_out.to_host(np.uint64, shape=(-1,))
    for buf in (d_org, d_cur, d_dj, d_out):
        buf.free()
    for (k, p, _), v in zip(items, out):
        assert int(got["results"][k]["sse"][p]) == int(v), (k, p)


def test_isp_chain_rejects_malformed_tables(ctx):
    for name, defect in isp.DEFECTS:
        b = isp.base_batch()
        defect(b)
        st, got = b.run_dev(ctx)
        assert st == lib.E_INVALID, name
        assert isp.Batch.untouched(got), name
