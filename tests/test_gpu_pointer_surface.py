"""The pointer surface (the entries that take host arrays) with PADDED host arrays: every block has a row stride of width + 3, the padding of an input holds
32767 / -32768 (a read past `width` changes the result) and the padding of an output holds a sentinel that must survive.  The Python wrappers hand the
library compact destinations, so the un-staging stride of these entries is not exercised anywhere else.

Expected values: numpy where the rule is a line (SAD with subShift, SSE, the masked SAD, the ICT through jccr_util, the LMCS rules through lmcs_util), otherwise
the batched _dev entry of the same operation on the same samples uploaded with the same strides (those kernels are pinned to the oracle by their own tests)."""
import ctypes as C

import numpy as np
import pytest

import jccr_util as ju
import lmcs_util as lu
import wp_util as wpu
import wtd_util as wu
from vtm_amd import lib
from vtm_amd.device import Context

pytestmark = pytest.mark.gpu

PAD, HI, LO, SENT = 3, 32767, -32768, -21846
SAD, SATD, SSE = 0, 1, 2
LUMA8 = [-1, 4, -11, 40, 40, -11, 4, -1]


def padded(rng, w, h, lo, hi, fill):
    """(h, w + PAD) int16: random samples in [lo, hi) and `fill` in the padding columns"""
    a = np.full((h, w + PAD), fill, np.int16)
    a[:, :w] = rng.integers(lo, hi, (h, w))
    return a


def out_block(w, h):
    return np.full((h, w + PAD), SENT, np.int16)


def check_out(dst, w, exp, what):
    assert (dst[:, w:] == SENT).all(), "%s: the destination's padding was written" % (what,)
    assert np.array_equal(dst[:, :w], exp), what


class Dev:
    """device buffers of one comparison, freed on exit"""

    def __init__(self, ctx):
        self.ctx, self.bufs = ctx, []

    def up(self, arr):
        self.bufs.append(self.ctx.to_device(arr))
        return self.bufs[-1].ptr

    def job(self, j):
        return self.up(np.frombuffer(bytes(j), np.uint8))

    def new(self, nbytes):
        self.bufs.append(self.ctx.alloc(nbytes))
        return self.bufs[-1]

    def __enter__(self):
        return self

    def __exit__(self, *a):
        for b in self.bufs:
            b.free()


def dev_dist(ctx, org, cur, w, h, kind, ss=0):
    with Dev(ctx) as d:
        out = d.new(8)
        ctx.dist_batch(d.up(org), d.up(cur), d.job(lib.DistJob(0, 0, org.shape[1], cur.shape[1], w, h, ss, kind)), 1, out.ptr)
        return int(out.to_host(np.uint64)[0])


def np_sad(org, cur, w, h, ss):
    o, c = org[:h:1 << ss, :w].astype(np.int64), cur[:h:1 << ss, :w].astype(np.int64)
    return int(np.abs(o - c).sum()) << ss


def np_sse(org, cur, w, h):
    d = org[:h, :w].astype(np.int64) - cur[:h, :w].astype(np.int64)
    return int((d * d).sum())


def dist_all(ctx, rng, w, h, ss=0, had=False):
    """the three plain distortions of one padded pair against numpy / the batched entry"""
    org, cur = padded(rng, w, h, 0, 1024, HI), padded(rng, w, h, 0, 1024, LO)
    s = w + PAD
    assert ctx.xGetSAD(org, s, cur, s, w, h, ss) == np_sad(org, cur, w, h, ss) == dev_dist(ctx, org, cur, w, h, SAD, ss), (w, h, ss)
    assert ctx.xGetSSE(org, s, cur, s, w, h) == np_sse(org, cur, w, h) == dev_dist(ctx, org, cur, w, h, SSE), (w, h)
    if had:
        assert ctx.xGetHADs(org, s, cur, s, w, h) == dev_dist(ctx, org, cur, w, h, SATD), (w, h)


@pytest.mark.parametrize("w,h,ss,had", [(1, 1, 0, False), (3, 5, 0, False), (8, 2, 1, True), (2, 2, 0, True), (16, 8, 0, True), (128, 128, 0, True)])
def test_plain_distortions(ctx, w, h, ss, had):
    dist_all(ctx, np.random.default_rng(100 * w + h), w, h, ss, had)


def masked_case(rng, w, h, step_x, mask_stride, mask_stride2, ss=0):
    """a mask plane whose walk (offsets r * rowStep + x * stepX from mask_off) is surrounded by 32767"""
    org, cur = padded(rng, w, h, 0, 1024, HI), padded(rng, w, h, 0, 1024, LO)
    row_step = w * step_x + mask_stride * (1 << ss) + mask_stride2
    offs = np.array([[r * row_step + x * step_x for x in range(w)] for r in range(h >> ss)])
    mask_off = 7 - int(offs.min())
    mask = np.full(mask_off + int(offs.max()) + 8, HI, np.int16)
    mask[mask_off + offs] = rng.integers(0, 9, offs.shape)
    exp = int((np.abs(org[:h:1 << ss, :w].astype(np.int64) - cur[:h:1 << ss, :w]) * mask[mask_off + offs]).sum()) << ss
    return org, cur, mask, mask_off, int(offs.min()), exp


@pytest.mark.parametrize("w,h,ss,step_x,mask_stride,mask_stride2", [(4, 4, 0, -1, 9, 0), (5, 3, 0, -1, 8, -20), (5, 3, 0, 1, 8, 0), (4, 4, 1, -1, 9, 0)])
def test_masked_sad(ctx, w, h, ss, step_x, mask_stride, mask_stride2):
    rng = np.random.default_rng(7 * w + h + ss)
    org, cur, mask, mask_off, lo, exp = masked_case(rng, w, h, step_x, mask_stride, mask_stride2, ss)
    assert step_x > 0 or lo < 0   # the walk starts at the high end of the plane
    s = w + PAD
    assert ctx.xGetSADwMask(org, s, cur, s, w, h, mask, mask_off, mask_stride, step_x, mask_stride2, ss) == exp
    with Dev(ctx) as d:
        out = d.new(8)
        job = lib.MaskedSadJob(0, 0, mask_off, s, s, mask_stride, mask_stride2, w, h, ss, step_x)
        ctx.masked_sad_batch(d.up(org), d.up(cur), d.up(mask), d.job(job), 1, out.ptr)
        assert int(out.to_host(np.uint64)[0]) == exp


@pytest.mark.parametrize("w,h,step_x,weight_stride", [(4, 4, -1, 11), (5, 3, -1, -9), (4, 4, -2, 13), (5, 3, -2, 16), (5, 3, 2, 16)])
def test_weighted_geo_blk(ctx, w, h, step_x, weight_stride):
    rng = np.random.default_rng(11 * w + h - step_x)
    src0, src1, dst = padded(rng, w, h, -4000, 12000, HI), padded(rng, w, h, -4000, 12000, LO), out_block(w, h)
    offs = np.array([[y * weight_stride + x * step_x for x in range(w)] for y in range(h)])
    w_off = 5 - int(offs.min())
    weight = np.full(w_off + int(offs.max()) + 6, HI, np.int16)
    weight[w_off + offs] = rng.integers(0, 9, offs.shape)
    assert step_x > 0 or offs.min() < 0
    s = w + PAD
    ctx._check(ctx.L.vtmhip_weightedGeoBlk(ctx.h, src0.ctypes.data, s, src1.ctypes.data, s, dst.ctypes.data, s, w, h, weight.ctypes.data + 2 * w_off, step_x,
                                           weight_stride, 10, 0, 1023))
    with Dev(ctx) as d:
        both, out = np.concatenate([src0.reshape(-1), src1.reshape(-1)]), d.new(2 * w * h)
        job = lib.GeoBlendJob(0, src0.size, 0, w_off, s, s, w, weight_stride, w, h, step_x, 0)
        ctx.weightedGeoBlk_batch(d.up(both), out.ptr, d.up(weight), d.job(job), 1, 10, (0, 1023))
        exp = out.to_host(np.int16).reshape(h, w)
    check_out(dst, w, exp, "weightedGeoBlk")
    # m_weightedGeoBlk itself, restated: ( w * s0 + ( 8 - w ) * s1 + offset ) >> shift with the 14-bit intermediates' offset
    wt = weight[w_off + offs].astype(np.int64)
    rule = np.clip((wt * (src0[:, :w].astype(np.int64) + 8192) + (8 - wt) * (src1[:, :w].astype(np.int64) + 8192) + 64) >> 7, 0, 1023)
    assert np.array_equal(exp, rule)


def filter_case(ctx, rng, vertical, taps, w, h, first, last):
    before, after = (taps // 2 - 1, taps // 2) if taps else (0, 0)
    sw, sh = w + (0 if vertical else before + after), h + (before + after if vertical else 0)
    src, dst = padded(rng, sw, sh, 0, 1024, HI), out_block(w, h)
    s, src_off = sw + PAD, (before * (sw + PAD) if vertical else before)
    co = np.array((LUMA8[4 - taps // 2:4 + taps // 2] if taps else []) + [0] * (8 - taps), np.int16)
    if taps == 0:
        ctx._check(ctx.L.vtmhip_filterCopy(ctx.h, first, last, src.ctypes.data + 2 * src_off, s, dst.ctypes.data, w + PAD, w, h, 10, 0, 1023, 0))
    else:
        fn = ctx.L.vtmhip_filterVer if vertical else ctx.L.vtmhip_filterHor
        ctx._check(fn(ctx.h, taps, first, last, src.ctypes.data + 2 * src_off, s, dst.ctypes.data, w + PAD, w, h, co.ctypes.data, 10, 0, 1023, 0))
    with Dev(ctx) as d:
        out = d.new(2 * w * h)
        job = lib.IfJob(src_off, 0, s, w, w, h, vertical, taps, first, last, (C.c_int16 * 8)(*co.tolist()), 0, 1023, 10, 0, 0, 0)
        ctx.if_batch(d.up(src), out.ptr, d.job(job), 1)
        exp = out.to_host(np.int16).reshape(h, w)
    check_out(dst, w, exp, ("filter", vertical, taps, w, h, first, last))
    return src[:, :sw], exp


def test_filter_ver_stages_the_extra_rows(ctx):
    src, got = filter_case(ctx, np.random.default_rng(1), 1, 8, 4, 1, 1, 1)      # 8 taps on 4x1: seven extra rows
    acc = (np.array(LUMA8, np.int64)[:, None] * src.astype(np.int64)).sum(axis=0)
    assert np.array_equal(got[0], np.clip((acc + 32) >> 6, 0, 1023))
    filter_case(ctx, np.random.default_rng(2), 1, 8, 4, 1, 1, 0)
    filter_case(ctx, np.random.default_rng(3), 1, 4, 3, 2, 0, 1)


def test_filter_hor_and_copy(ctx):
    src, got = filter_case(ctx, np.random.default_rng(4), 0, 8, 1, 4, 1, 1)      # 8 taps on 1x4: seven extra columns
    acc = (src.astype(np.int64) * np.array(LUMA8, np.int64)[None, :]).sum(axis=1)
    assert np.array_equal(got[:, 0], np.clip((acc + 32) >> 6, 0, 1023))
    filter_case(ctx, np.random.default_rng(5), 0, 2, 5, 3, 1, 0)
    src, got = filter_case(ctx, np.random.default_rng(6), 0, 0, 3, 3, 1, 1)
    assert np.array_equal(got, src)
    filter_case(ctx, np.random.default_rng(7), 0, 0, 3, 3, 1, 0)


@pytest.mark.parametrize("signal", [wu.SDR, wu.PQ])
def test_sse_wtd_chroma_with_padded_luma(ctx, signal):
    rng = np.random.default_rng(30 + signal)
    bd, w, h, sx, sy = 10, 2, 2, 1, 1
    lut, cw = wu.random_table(rng, bd), 1.37
    ctx.set_luma_level_weights(lut, bd, signal, cw)
    org, cur, luma = padded(rng, w, h, 0, 1024, HI), padded(rng, w, h, 0, 1024, LO), padded(rng, w << sx, h << sy, 0, 1024, HI)
    luma[1::2, :] = HI      # the rows between the co-located ones are never read (a weight-table index of 32767 would be)
    s, ls = w + PAD, (w << sx) + PAD
    for comp in (1, 2):
        got = ctx.xGetSSE_WTD(org, s, cur, s, w, h, comp, luma, ls, sx, sy)
        assert got == wu.sse_wtd(org[:, :w], cur[:, :w], comp, lut, signal, cw, luma, sx, sy)
        with Dev(ctx) as d:
            out = d.new(8)
            jobs = wu.pack_jobs([dict(orgOff=0, curOff=0, orgLumaOff=0, orgStride=s, curStride=s, orgLumaStride=ls, width=w, height=h, compID=comp, cShiftX=sx, cShiftY=sy,
                                      flags=0)])
            ctx.sse_wtd_batch(d.up(org), d.up(cur), d.up(luma), d.up(jobs), 1, out.ptr)
            assert int(out.to_host(np.uint64)[0]) == got
    assert ctx.xGetSSE_WTD(org, s, cur, s, w, h, 0) == wu.sse_wtd(org[:, :w], cur[:, :w], 0, lut, signal, cw)


@pytest.mark.parametrize("w,h", [(4, 2), (2, 2)])
def test_weighted_prediction_distortions(ctx, w, h):
    rng = np.random.default_rng(40 + w)
    bd, s = 10, w + PAD
    for bi in (0, 1):
        wp = wpu.random_wp(rng, bd)
        org, cur = padded(rng, w, h, 0, 1024, HI), padded(rng, w, h, 0, 1024, LO)
        got = (ctx.xGetSADw(org, s, cur, s, w, h, wp, bd, bi), ctx.xGetHADsw(org, s, cur, s, w, h, wp, bd, bi), ctx.xGetSSEw(org, s, cur, s, w, h, wp, bd, bi))
        with Dev(ctx) as d:
            out = d.new(24)
            jobs = wpu.pack_dist_jobs([dict(orgOff=0, curOff=0, orgStride=s, curStride=s, width=w, height=h, kind=k, bitDepth=bd, isBiPred=bi, wp=wp, maxDist=wpu.U64)
                                       for k in (SAD, SATD, SSE)])
            ctx.wp_dist_batch(d.up(org), d.up(cur), d.up(jobs), 3, out.ptr)
            assert got == tuple(int(v) for v in out.to_host(np.uint64)), (w, h, bi)
        o, c = np.ascontiguousarray(org[:, :w]), np.ascontiguousarray(cur[:, :w])
        assert got == tuple(wpu.dist_w(k, o, c, wp, bd, bi) for k in (SAD, SATD, SSE)), (w, h, bi)


def in_place_view(rng, w, h, lo, hi, fill):
    """a w x h block inside a larger array (one row above and below, two columns left, PAD right) filled with `fill`"""
    big = np.full((h + 2, w + 2 + PAD), fill, np.int16)
    big[1:1 + h, 2:2 + w] = rng.integers(lo, hi, (h, w))
    return big, big[1:1 + h, 2:2 + w]


def check_in_place(big, before, w, h, exp, what):
    after = before.copy()
    after[1:1 + h, 2:2 + w] = exp
    assert np.array_equal(big, after), what


@pytest.mark.parametrize("w,h", [(3, 2), (8, 8)])
def test_lmcs_signals_in_place(ctx, w, h):
    rng = np.random.default_rng(50 + w)
    lut = lu.make_lut(5, 10)
    big, blk = in_place_view(rng, w, h, 0, 1024, HI)
    before = big.copy()
    ctx.rspSignal(blk, lut)
    check_in_place(big, before, w, h, lu.rsp_signal(before[1:1 + h, 2:2 + w], lut), ("rspSignal", w, h))
    for fwd, scale in ((1, 1500), (0, 2731), (1, 32767), (0, 1)):
        big, blk = in_place_view(rng, w, h, -1024, 1024, LO)
        before = big.copy()
        ctx.scaleSignal(blk, scale, fwd, 10)
        check_in_place(big, before, w, h, lu.scale_signal(before[1:1 + h, 2:2 + w], scale, fwd, 10), ("scaleSignal", w, h, fwd, scale))
    # a sample outside the LUT: refused, and nothing is written
    big, blk = in_place_view(rng, w, h, 0, 1024, HI)
    blk[h - 1, w - 1] = 1024
    before = big.copy()
    with pytest.raises(lib.VtmHipError, match="outside the LUT"):
        ctx.rspSignal(blk, lut)
    assert np.array_equal(big, before)


@pytest.mark.parametrize("mode", [0, 1, -1, 2, -2, 3, -3])
def test_fwd_transform_cbcr(ctx, mode):
    rng = np.random.default_rng(60 + mode)
    w, h, s = 4, 2, 4 + PAD
    cb, cr, c1, c2 = padded(rng, w, h, -2000, 2000, HI), padded(rng, w, h, -2000, 2000, LO), out_block(w, h), out_block(w, h)
    d = (C.c_int64 * 2)()
    ctx._check(ctx.L.vtmhip_fwdTransformCbCr(ctx.h, mode, cb.ctypes.data, s, cr.ctypes.data, s, c1.ctypes.data, s, c2.ctypes.data, s, w, h, d))
    joint, dist = ju.fwd_ict(mode, cb[:, :w], cr[:, :w])
    assert (d[0], d[1]) == dist
    used, other = (c2, c1) if abs(mode) == 3 else (c1, c2)
    assert (other == SENT).all()
    if mode:
        check_out(used, w, joint, ("fwdTransformCbCr", mode))
    else:
        assert (used == SENT).all()


@pytest.mark.parametrize("mode", [1, -1, 2, -2, 3, -3])
def test_inv_transform_cbcr_in_place(ctx, mode):
    rng = np.random.default_rng(70 + mode)
    w, h = 4, 2
    bcb, cb = in_place_view(rng, w, h, -2000, 2000, HI)
    bcr, cr = in_place_view(rng, w, h, -2000, 2000, LO)
    cb0, cr0 = bcb.copy(), bcr.copy()
    ecb, ecr = ju.inv_ict(mode, cb0[1:1 + h, 2:2 + w], cr0[1:1 + h, 2:2 + w])
    ctx.invTransformCbCr(mode, cb, cr)
    check_in_place(bcb, cb0, w, h, ecb, ("invTransformCbCr cb", mode))
    check_in_place(bcr, cr0, w, h, ecr, ("invTransformCbCr cr", mode))
    untouched, orig = (bcr, cr0) if abs(mode) == 3 else (bcb, cb0)
    assert untouched.tobytes() == orig.tobytes()      # the component the mode does not derive stays bit-identical


def test_staging_area_grows_in_the_middle_of_a_sequence():
    """a fresh context: small calls, a 128x128 call, a call whose mask walk needs more than the staging area holds (it grows), then small calls again"""
    rng = np.random.default_rng(80)
    with Context(0) as c:
        dist_all(c, rng, 3, 5)
        filter_case(c, rng, 1, 8, 4, 1, 1, 1)
        dist_all(c, rng, 128, 128, had=True)
        dist_all(c, rng, 8, 2, 1, True)
        w, h, stride = 4, 4, 300000                    # 3 rows x 300000 samples x 2 bytes: beyond the first MiB
        org, cur, mask, mask_off, lo, exp = masked_case(rng, w, h, -1, stride, 0)
        assert mask.nbytes > 1 << 20 and lo < 0
        assert c.xGetSADwMask(org, w + PAD, cur, w + PAD, w, h, mask, mask_off, stride, -1, 0) == exp
        dist_all(c, rng, 1, 1)
        filter_case(c, rng, 0, 8, 1, 4, 1, 1)
        big, blk = in_place_view(rng, 3, 2, -1024, 1024, LO)
        before = big.copy()
        c.scaleSignal(blk, 1500, 1, 10)
        check_in_place(big, before, 3, 2, lu.scale_signal(before[1:3, 2:5], 1500, 1, 10), "scaleSignal after the growth")
