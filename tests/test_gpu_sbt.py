"""GPU parity of the sub-block transform (SBT) entries: vtmhip_sbt_est_batch_dev (InterSearch::calcMinDistSbt) on its three launch shapes and
vtmhip_sbt_chain_batch_dev (the SBT candidates of xEstimateInterResidualQT) on the generic and the bucketed path of the fused chain, at 8 / 10 / 12 bits --
against the Python restatement of the reference's rules (tests/sbt_util.py, pinned to the real members in tests/test_sbt.py), the oracle's transform steps and
the recorded reference results (tests/golden/sbt.npz).  Bit-exact."""
import ctypes as C

import numpy as np
import pytest

import sbt_util as su
from vtm_amd import lib
from vtm_amd.lib import SbtJob, SbtResult, TuJob, TuResult, VtmHipError

pytestmark = pytest.mark.gpu

EST_SHAPES = [(4, 8), (8, 4), (8, 8), (16, 8), (8, 16), (16, 16), (64, 16), (16, 64), (64, 64)]
CHAIN_SHAPES = EST_SHAPES + [(32, 32), (64, 32), (32, 64)]
SKIP_THRESHOLD = float(12 << 15)


def _est_specs(rng, shapes, bd, reps=1):
    """every shape luma-only and with chroma, on both sides of the skipAll threshold (distScale placed from the samples' own SSE) and at an encoder's distScale"""
    specs = []
    for _ in range(reps):
        for (w, h) in shapes:
            for chroma in (False, True):
                for factor in (0.6, 1.7, None):
                    s = su.est_spec(rng, w, h, bd, chroma, amp=int(rng.choice([2, 30, (1 << bd) - 1])), cw=float(rng.choice([0.8137, 1.0 / 3.0, 1.2589])))
                    if factor is not None:
                        total = sum(int(((o.astype(np.int64) - p) ** 2).sum()) for o, p in s["blocks"])
                        s["ds"] = SKIP_THRESHOLD / max(total, 1) * factor
                    specs.append(s)
    return specs


@pytest.fixture(scope="module")
def est_batches():
    """one batch per bit depth, shared by the estimator tests (the expectations are computed once)"""
    return {bd: su.EstBatch(_est_specs(np.random.default_rng(40 + bd), EST_SHAPES, bd), seed=bd) for bd in (8, 10, 12)}


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_estimator_every_launch_shape(ctx, est_batches, bd):
    """16 lanes per CU (CUs up to 256 luma samples), a wave per CU (up to 1024), a workgroup per CU; batch sizes 1, a few, all"""
    b = est_batches[bd]
    skips = [e["skipAll"] for e in b.exp]
    assert 0 in skips and 1 in skips and sum(skips) * 4 >= len(skips) and (len(skips) - sum(skips)) * 4 >= len(skips)   # both sides of the threshold
    assert any(s["chroma"] for s in b.specs) and any(not s["chroma"] for s in b.specs)
    for limit in (256, 1024, 4096):
        idx = [k for k, s in enumerate(b.specs) if s["w"] * s["h"] <= limit]
        assert max(b.specs[k]["w"] * b.specs[k]["h"] for k in idx) == limit
        b.check(b.run(ctx, idx), idx)
        b.check(b.run(ctx, idx[-1:]), idx[-1:])
        b.check(b.run(ctx, idx[3:8]), idx[3:8])


def test_estimator_several_hundred_mixed_jobs(ctx):
    rng = np.random.default_rng(7)
    specs = []
    for bd in (8, 10, 12):   # a job carries its own bit depth
        specs += _est_specs(rng, EST_SHAPES, bd, reps=2)
    order = rng.permutation(len(specs))
    b = su.EstBatch([specs[k] for k in order], seed=3)
    assert b.n >= 300 and len({e["skipAll"] for e in b.exp}) == 2
    b.check(b.run(ctx))


def test_estimator_tie_goes_to_the_lower_mode(ctx):
    """a residual mirrored left to right with its energy in the top rows: HOR_H0 is the best half mode, VER_H0 and VER_H1 tie for the second place"""
    rng = np.random.default_rng(11)
    left = np.concatenate([rng.integers(100, 200, (8, 8)), rng.integers(0, 4, (8, 8))])
    d = np.concatenate([left, left[:, ::-1]], axis=1)
    org = rng.integers(300, 700, (16, 16))
    spec = dict(w=16, h=16, bd=10, chroma=False, allowed=su.sbt_allowed(16, 16), cw=1.0, ds=1.0, blocks=[(org.astype(np.int16), (org - d).astype(np.int16))])
    b = su.EstBatch([spec])
    e = b.exp[0]
    assert e["skipAll"] == 0 and e["est"][0] == e["est"][1] and e["est"][4] == e["est"][5] and e["order"][:2] == [2, 0] and e["order"][2:4] == [6, 4], e
    b.check(b.run(ctx))


def test_estimator_skips_invalid_jobs_and_checks_arguments(ctx):
    rng = np.random.default_rng(12)
    b = su.EstBatch([su.est_spec(rng, 16, 16, 10, True, 30), su.est_spec(rng, 8, 8, 10, True, 30), su.est_spec(rng, 16, 16, 10, True, 30)])
    b.jobs[1].sbtAllowed = 1 << su.VER_QUAD   # an 8-wide CU has no quarter split
    res = b.run(ctx)
    b.check([res[0], res[2]], [0, 2])
    assert bytes(res[1]) == b"\xa5" * C.sizeof(lib.SbtEstResult)   # a job outside the contract is skipped: its record is not written
    with pytest.raises(VtmHipError):
        ctx.sbt_est_batch(None, 1, 1, 1, 16, 16, 1)
    with pytest.raises(VtmHipError):
        ctx.sbt_est_batch(1, 1, 1, 1, 128, 16, 1)
    ctx.sbt_est_batch(None, None, None, 0, 16, 16, None)


# ---- the candidate chain -------------------------------------------------------------------------------------------------------------------------------
def _chain_specs(rng, bds, reps=1):
    """every shape x every allowed mode; QP 22 / 32 / 42, slice type and the presence of chroma rotate; every fourth candidate has a residual of +-1 at QP 42,
    which quantises to nothing"""
    specs, k = [], 0
    for _ in range(reps):
        for (w, h) in CHAIN_SHAPES:
            for mode in su.allowed_modes(w, h):
                bd = bds[k % len(bds)]
                quiet = k % 4 == 3
                specs.append(su.chain_spec(rng, w, h, mode, bd, 42 if quiet else (22, 32, 42)[(k // 2) % 3], k % 2, k % 3 != 2, 1 if quiet else 60 << (bd - 8)))
                k += 1
    return specs


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_chain_generic_path(ctx, bd):
    """fewer than 256 sub-TUs: the generic kernel of the fused chain.  Every shape and allowed mode, chroma down to 2x2."""
    b = su.ChainBatch(_chain_specs(np.random.default_rng(20 + bd), [bd]), seed=bd)
    tiles = [e["tile"][2:] for es in b.exp for e in es if e is not None]
    assert len(tiles) < 256 and (2, 2) in tiles and (16, 64) in tiles and (64, 16) in tiles and (32, 32) in tiles
    types = {(es[0]["tile"][2:], es[0]["types"]) for es in b.exp}
    assert ((16, 64), (su.DCT2, su.DCT2)) in types and ((64, 16), (su.DCT2, su.DCT2)) in types and ((32, 16), (su.DCT8, su.DST7)) in types and ((16, 32), (su.DST7, su.DCT8)) in types
    assert {s["qp"] for s in b.specs} == {22, 32, 42}
    b.assert_bites()
    b.check(b.run(ctx))


def test_chain_bucketed_path(ctx):
    """a mixed batch of more than 256 candidates at all three bit depths: the fused chain buckets the sub-TUs by shape"""
    b = su.ChainBatch(_chain_specs(np.random.default_rng(31), [8, 10, 12], reps=4), seed=5)
    tiles = [e["tile"][2:] for es in b.exp for e in es if e is not None]
    assert b.n >= 256 and any(min(t) >= 8 for t in tiles) and any(min(t) == 4 for t in tiles) and any(min(t) == 2 for t in tiles) and max(max(t) for t in tiles) == 64
    b.assert_bites()
    got = b.run(ctx)
    b.check(got)
    # the optional outputs: without them the results are the same and nothing is written
    res2, lv2, rec2 = b.run(ctx, levels=False, rec=False)
    assert bytes(res2) == bytes(got[0]) and (lv2 == -7).all() and (rec2 == -7).all()
    b.check(b.run(ctx, idx=[5, 200, 17], rec=False), idx=[5, 200, 17], rec=False)


def test_chain_luma_equals_the_plain_chain_on_the_hand_built_sub_tu(ctx):
    """a 32x16 CU, VER_HALF POS1: the right 16x16 half with DST-7 / DST-7 -- the candidate's luma result is vtmhip_tu_chain_batch_dev's on that job"""
    rng = np.random.default_rng(41)
    b = su.ChainBatch([su.chain_spec(rng, 32, 16, 1, 10, 27, 0, False, 200)])
    res, lv, rec = b.run(ctx)
    j = b.jobs[0]
    t = (TuJob * 1)()
    t[0].resiOff, t[0].outOff, t[0].resiStride, t[0].width, t[0].height = j.resiOff[0] + 16, 0, j.resiStride[0], 16, 16
    t[0].qpPer, t[0].qpRem, t[0].typeHor, t[0].typeVer, t[0].bitDepth, t[0].isIRAP = j.qpPer[0], j.qpRem[0], lib.DST7, lib.DST7, 10, 0
    d_resi, d_t, d_r = ctx.to_device(b.resi), ctx.to_device(np.frombuffer(t, np.uint8)), ctx.alloc(C.sizeof(TuResult))
    d_lv, d_rec = ctx.alloc(4 * 256, np.int32), ctx.alloc(2 * 256, np.int16)
    ctx.tu_chain_batch(d_resi.ptr, d_t.ptr, 1, 16, 16, d_r.ptr, d_lv.ptr, d_rec.ptr)
    r = TuResult.from_buffer_copy(d_r.to_host(np.uint8).tobytes())
    assert r.absSum > 0 and (res[0].sseCoded[0], res[0].absSum[0]) == (r.sse, r.absSum)
    assert np.array_equal(lv[0, 7:7 + 256], d_lv.to_host())
    assert np.array_equal(rec[0, 7:7 + 512].reshape(16, 32)[:, 16:], d_rec.to_host().reshape(16, 16)) and (rec[0, 7:7 + 512].reshape(16, 32)[:, :16] == 0).all()
    b.check((res, lv, rec))
    for d in (d_resi, d_t, d_r, d_lv, d_rec):
        d.free()


def test_chain_replays_the_recorded_reference(ctx):
    """tests/golden/sbt.npz through the device: the real members' levels, reconstructed sub-TU, SSE and absSum; the partition sums through the estimator"""
    rng = np.random.default_rng(51)
    cases = list(su.golden_cases())
    specs = []
    for g in cases:
        filler = rng.integers(-50, 51, (g["h"], g["w"])).astype(np.int16)
        resi = [g["resi"]] if g["luma"] else [filler, g["resi"], g["resi"]]
        specs.append(dict(w=g["w"], h=g["h"], mode=g["mode"], bd=g["bd"], qp=g["qp"], qpc=g["qp"], irap=g["irap"], chroma=not g["luma"], resi=resi))
    b = su.ChainBatch(specs)
    res, lv, rec = got = b.run(ctx)
    b.check(got)
    for k, g in enumerate(cases):
        for c in ((0,) if g["luma"] else (1, 2)):
            x, y, tw, th = b.exp[k][c]["tile"]
            cw, ch = su.comp_shape(g["w"], g["h"], c)
            assert (res[k].sseCoded[c], res[k].absSum[c]) == (g["sse"], g["absSum"]), (k, c)
            assert np.array_equal(lv[3 * k + c, 7:7 + tw * th], g["levels"]), (k, c)
            assert np.array_equal(rec[3 * k + c, 7:7 + cw * ch].reshape(ch, cw)[y:y + th, x:x + tw], g["rec_sub"]), (k, c)
    # the recorded partition SSEs: the residual as `org` against a zero prediction
    est = []
    for g in cases:
        if g["luma"]:
            est.append(dict(w=g["w"], h=g["h"], bd=g["bd"], chroma=False, allowed=su.sbt_allowed(g["w"], g["h"]), cw=1.0, ds=1.0, blocks=[(g["resi"], np.zeros_like(g["resi"]))]))
    eb = su.EstBatch(est)
    out = eb.run(ctx)
    eb.check(out)
    for r, g in zip(out, [g for g in cases if g["luma"]]):
        assert [list(r.part[0][j]) for j in range(4)] == g["part"]


def test_chain_argument_errors_launch_nothing(ctx):
    rng = np.random.default_rng(61)
    b = su.ChainBatch([su.chain_spec(rng, 16, 16, m, 10, 32, 0, True, 100) for m in (0, 3, 5)])

    def attempt(change):
        sub = b.sub_jobs()
        change(sub[1])
        d_resi, d_jobs = ctx.to_device(b.resi), ctx.to_device(np.frombuffer(sub, np.uint8))
        d_res = ctx.to_device(np.full(C.sizeof(SbtResult) * 3, 0xA5, np.uint8))
        d_lv, d_rec = ctx.to_device(np.full(9 * b.SLOT, -7, np.int32)), ctx.to_device(np.full(9 * b.SLOT, -7, np.int16))
        with pytest.raises(VtmHipError):
            ctx.sbt_chain_batch(d_resi.ptr, d_jobs.ptr, 3, d_res.ptr, d_lv.ptr, d_rec.ptr)
        assert (d_res.to_host(np.uint8) == 0xA5).all() and (d_lv.to_host() == -7).all() and (d_rec.to_host() == -7).all()
        for d in (d_resi, d_jobs, d_res, d_lv, d_rec):
            d.free()

    def setter(field, value, c=None):
        def f(j):
            if c is None:
                setattr(j, field, value)
            else:
                getattr(j, field)[c] = value
        return f

    for ch in (setter("sbtIdx", 0), setter("sbtIdx", 5), setter("sbtPos", 2), setter("width", 12), setter("height", 128), setter("width", 2),
               setter("bitDepth", 13), setter("qpRem", 6, 0), setter("qpPer", -1, 2), setter("resiOff", -1, 0)):
        attempt(ch)
    j = SbtJob()
    C.memmove(C.byref(j), C.byref(b.jobs[2]), C.sizeof(SbtJob))
    j.width = 8   # VER_QUAD on an 8-wide CU: a mode the size does not allow
    d_jobs, d_res = ctx.to_device(np.frombuffer(j, np.uint8)), ctx.to_device(np.full(C.sizeof(SbtResult), 0xA5, np.uint8))
    with pytest.raises(VtmHipError):
        ctx.sbt_chain_batch(1, d_jobs.ptr, 1, d_res.ptr)
    assert (d_res.to_host(np.uint8) == 0xA5).all()
    with pytest.raises(VtmHipError):
        ctx.sbt_chain_batch(1, d_jobs.ptr, 1, None)       # NULL result pointer
    with pytest.raises(VtmHipError):
        ctx.sbt_chain_batch(None, d_jobs.ptr, 1, d_res.ptr)
    ctx.sbt_chain_batch(None, None, 0, None)              # n == 0: nothing to do
    b.check(b.run(ctx))                                   # and the untouched table still runs
