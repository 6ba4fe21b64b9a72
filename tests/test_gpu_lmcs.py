"""GPU parity of the LMCS residual path: the two pointer entries and the batched scaleSignal, the mapped-domain residual / reconstruction ops, and the
plain and the joint chain with chroma residual scaling fused in, on every launch path at 8 / 10 / 12 bits -- against the numpy restatement of the
reference's rules (tests/lmcs_util.py, itself pinned to the real members in tests/test_lmcs.py), the recorded reference results
(tests/golden/lmcs.npz) and the oracle's transform steps.  Bit-exact."""
import ctypes as C

import numpy as np
import pytest

import jccr_util as ju
import lmcs_util as lu
from vtm_amd import lib
from vtm_amd.device import Context
from vtm_amd.lib import JccrJob, JccrResult, LmcsJob, ScaleJob, TuResult, VtmHipError

pytestmark = pytest.mark.gpu

TU_FIELDS, JC_FIELDS = ("sse", "sumAbs", "absSum"), ("sseCb", "sseCr", "fwdDist", "sumAbs", "absSum")
SIGNED_MODES = [1, -1, 2, -2, 3, -3]
ADJS = [256, 300, 512, 1024, 1500, 2048, 2731, 4096, 16384, 0]   # ChromaScaleCoeff lies in 256 .. 16384; 0: this job is not scaled


def _strided(rng, blk, extra):
    h, w = blk.shape
    buf = rng.integers(-32768, 32768, (h, w + extra)).astype(np.int16)
    buf[:, 1:1 + w] = blk
    return buf, buf[:, 1:1 + w]


# ---- pointer entries and the batched scaleSignal ------------------------------------------------------------------------------------------------------
def test_pointer_entries_replay_the_recorded_reference(ctx):
    """vtmhip_scaleSignal / vtmhip_rspSignal on strided host blocks against tests/golden/lmcs.npz; samples outside the block stay as they were."""
    rng = np.random.default_rng(3)
    for w, h, bd, fwd, scale, blk, out in lu.golden_scale_cases():
        buf, view = _strided(rng, blk, 3)
        keep = buf.copy()
        ctx.scaleSignal(view, scale, fwd, bd)
        assert np.array_equal(view, out), (w, h, bd, fwd, scale)
        keep[:, 1:1 + w] = out
        assert np.array_equal(buf, keep), "samples outside the block were touched"
    z = lu.golden()
    for k in range(len(z["rsp_w"])):
        w, h, bd, o = int(z["rsp_w"][k]), int(z["rsp_h"][k]), int(z["rsp_bd"][k]), int(z["rsp_off"][k])
        lut = z["rsp_lut"][(bd - 8) // 2][:1 << bd]
        buf, view = _strided(rng, z["rsp_in"][o:o + w * h].reshape(h, w), 5)
        ctx.rspSignal(view, lut)
        assert np.array_equal(view, z["rsp_out"][o:o + w * h].reshape(h, w)), (w, h, bd)
    # the reference's THROW and an index outside the table
    col = np.full((4, 1), 7, np.int16)
    with pytest.raises(VtmHipError):
        ctx.scaleSignal(col, 2048, 1, 10)
    ctx.scaleSignal(col, 4096, 0, 10)
    assert col.reshape(-1).tolist() == [14] * 4
    for bad in (-1, 16):
        blk = np.array([[0, 15], [bad, 3]], np.int16)
        with pytest.raises(VtmHipError):
            ctx.rspSignal(blk, np.arange(16, dtype=np.int16))
        assert blk.tolist() == [[0, 15], [bad, 3]]
    for scale, bd in ((0, 10), (32768, 10), (2048, 7), (2048, 13)):
        with pytest.raises(VtmHipError):
            ctx.scaleSignal(np.zeros((4, 4), np.int16), scale, 1, bd)


def _scale_batch(ctx, src, w, h, scales, dirs, bd, in_place=False):
    """one launch: job k scales the block at src[0 : w * h] (in_place: its own copy) with scales[k] / dirs[k]; returns the n output blocks"""
    n, blk = len(scales), w * h
    jobs = (ScaleJob * n)()
    for k in range(n):
        j = jobs[k]
        j.srcOff, j.dstOff, j.srcStride, j.dstStride, j.width, j.height = (k * blk if in_place else 0), k * blk, w, w, w, h
        j.scale, j.dir, j.bitDepth = int(scales[k]), int(dirs[k]), bd
    d_jobs = ctx.to_device(np.frombuffer(jobs, np.uint8))
    if in_place:
        d_dst = ctx.to_device(np.tile(src, n))
        ctx.scale_signal_batch(d_dst.ptr, d_dst.ptr, d_jobs.ptr, n)
    else:
        d_src, d_dst = ctx.to_device(src), ctx.to_device(np.full(n * blk, 0x5555, np.int16))
        ctx.scale_signal_batch(d_src.ptr, d_dst.ptr, d_jobs.ptr, n)
    out = d_dst.to_host(np.int16).reshape(n, blk)
    d_jobs.free(), d_dst.free()
    return out


def _scale_expect(src, scales, dirs, bd):
    out = np.empty((len(scales), src.size), np.int16)
    for k0 in range(0, len(scales), 4096):       # in slices: the broadcast intermediates are int64
        s = np.asarray(scales[k0:k0 + 4096], np.int64).reshape(-1, 1)
        f, i = lu.scale_signal(src.reshape(1, -1), s, 1, bd), lu.scale_signal(src.reshape(1, -1), s, 0, bd)
        out[k0:k0 + 4096] = np.where(np.asarray(dirs[k0:k0 + 4096]).reshape(-1, 1) == 1, f, i)
    return out


def test_scale_signal_batch_every_scale(ctx):
    """One launch: every scale 1 .. 32767 in both directions against 256 samples (0 .. 64, 2^k - 1, 2^k, 2^k + 1 up to 4096, +-32767, -32768, both signs)."""
    vals = [v for v in lu.EDGE_VALUES if v <= 32767] + [-v for v in lu.EDGE_VALUES if v > 0]
    rng = np.random.default_rng(11)
    src = np.array(vals + rng.integers(-32768, 32768, 256 - len(vals)).tolist(), np.int16)
    assert src.size == 256 and {0, 64, 4095, 4096, 4097, 32767, -32767, -32768} <= set(src.tolist())
    scales, dirs = np.tile(np.arange(1, 32768), 2), np.repeat([1, 0], 32767)
    got = _scale_batch(ctx, src, 16, 16, scales, dirs, 12)
    exp = _scale_expect(src, scales, dirs, 12)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, (len(bad), [(int(scales[k]), int(dirs[k]), int(src[i]), int(got[k, i]), int(exp[k, i])) for k, i in bad[:5]])


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_scale_signal_batch_every_residual(ctx, bd):
    """Another launch: every |v| <= 4095 against 128 scales (the 256 .. 16384 edges, powers of two +-1, primes), both directions, in place, 128 x 64 blocks."""
    src = np.concatenate([np.arange(-4095, 4096), [4096]]).astype(np.int16)
    scales = (lu.EDGE_SCALES + [300, 1000, 3000, 5000, 6000, 7000, 9000, 10000, 12000, 14000, 15000, 20000, 25000, 30000] * 8)[:128]
    assert len(scales) == 128 and src.size == 128 * 64
    got = _scale_batch(ctx, src, 128, 64, scales * 2, [1] * 128 + [0] * 128, bd, in_place=True)
    assert np.array_equal(got, _scale_expect(src, scales * 2, [1] * 128 + [0] * 128, bd))


def test_scale_signal_batch_golden_and_rejects(ctx):
    """The recorded cases as one mixed launch (shapes 2x2 .. 16x16, strides wider than the block), and jobs outside the contract are skipped."""
    cases = list(lu.golden_scale_cases())
    n, stride = len(cases), 19
    src = np.full((n * 16, stride), 0x2222, np.int16)
    jobs = (ScaleJob * (n + 4))()
    for k, (w, h, bd, fwd, scale, blk, _out) in enumerate(cases):
        src[k * 16:k * 16 + h, 1:1 + w] = blk
        j = jobs[k]
        j.srcOff = j.dstOff = k * 16 * stride + 1
        j.srcStride, j.dstStride, j.width, j.height, j.scale, j.dir, j.bitDepth = stride, stride, w, h, scale, fwd, bd
    for i, (w, scale, d, bd) in enumerate([(1, 2048, 1, 10), (4, 0, 1, 10), (4, 40000, 0, 10), (4, 2048, 1, 13)]):   # width 1 forward, scale 0, scale > 32767, bit depth
        j = jobs[n + i]
        j.srcOff = j.dstOff = 0
        j.srcStride, j.dstStride, j.width, j.height, j.scale, j.dir, j.bitDepth = stride, stride, w, 1, scale, d, bd
    exp = src.copy()
    for k, (w, h, *_rest, out) in enumerate(cases):   # (the rejected jobs point at job 0's rows: those come out as job 0 alone leaves them)
        exp[k * 16:k * 16 + h, 1:1 + w] = out
    d_src, d_dst = ctx.to_device(src), ctx.to_device(src)
    ctx.scale_signal_batch(d_src.ptr, d_dst.ptr, ctx.to_device(np.frombuffer(jobs, np.uint8)).ptr, n + 4)
    assert np.array_equal(d_dst.to_host(np.int16).reshape(src.shape), exp)


# ---- resi / reco ------------------------------------------------------------------------------------------------------------------------------------
LUMA_SHAPES = [(1, 1), (2, 2), (4, 4), (8, 4), (16, 16), (64, 64), (128, 128), (12, 20)]


def _place(rng, cur, w, h):
    """an odd stride and an odd offset for a w x h block behind `cur`: (offset, stride, next cursor)"""
    stride = w + 1 + 2 * int(rng.integers(0, 4)) + (w & 1)
    stride += 1 - (stride & 1)
    off = cur + 1 + 2 * int(rng.integers(0, 3)) - (cur & 1) + 1
    off += 1 - (off & 1)
    return off, stride, off + stride * h + 3


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_lmcs_resi_and_reco(bd):
    """resi = fwdLUT[org] - (MAP_PRED ? fwdLUT[pred] : pred) with and without the mapped-prediction output, reco = clip(pred' + resi): shapes 1x1 .. 128x128 and
    12x20 at odd strides and offsets, a seeded monotone 16-piece LUT.  Samples outside the blocks keep their sentinel; the entries fail before the setter."""
    rng = np.random.default_rng(500 + bd)
    lut = lu.make_lut(40 + bd, bd)
    specs, cur = [], [0, 0, 0, 0]
    for (w, h) in LUMA_SHAPES:
        for flags in (0, lu.MAP_PRED, lu.WRITE_MAPPED, lu.MAP_PRED | lu.WRITE_MAPPED):
            pl = []
            for b in range(4):
                off, stride, cur[b] = _place(rng, cur[b], w, h)
                pl.append((off, stride))
            specs.append((w, h, flags, pl))
    size = max(cur) + 8
    top = (1 << bd) - 1
    org, pred = rng.integers(0, top + 1, size).astype(np.int16), rng.integers(0, top + 1, size).astype(np.int16)
    rin = rng.integers(-top, top + 1, size).astype(np.int16)
    n = len(specs)
    jobs = (LmcsJob * n)()
    exp_resi, exp_dst, exp_reco = np.full(size, 0x3333, np.int16), np.full(size, 0x4444, np.int16), np.full(size, 0x6666, np.int16)

    def view(a, off, stride, w, h):
        return np.lib.stride_tricks.as_strided(a[off:], (h, w), (2 * stride, 2))

    for k, (w, h, flags, pl) in enumerate(specs):
        j = jobs[k]
        (j.orgOff, j.orgStride), (j.predOff, j.predStride), (j.resiOff, j.resiStride), (j.dstOff, j.dstStride) = pl
        j.width, j.height, j.bitDepth, j.flags = w, h, bd, flags
        o, p = view(org, *pl[0], w, h), view(pred, *pl[1], w, h)
        r, mapped = lu.resi_expect(o, p, lut, flags & lu.MAP_PRED)
        view(exp_resi, *pl[2], w, h)[:] = r
        if flags & lu.WRITE_MAPPED:
            view(exp_dst, *pl[3], w, h)[:] = mapped
        if not flags & lu.WRITE_MAPPED:          # the reco jobs: the two MAP_PRED settings of every shape
            view(exp_reco, *pl[3], w, h)[:] = lu.reco_expect(p, view(rin, *pl[2], w, h), lut, flags & lu.MAP_PRED, bd)
    with Context(0) as c:
        d_org, d_pred, d_rin, d_jobs = c.to_device(org), c.to_device(pred), c.to_device(rin), c.to_device(np.frombuffer(jobs, np.uint8))
        d_resi, d_dst, d_reco = c.to_device(np.full(size, 0x3333, np.int16)), c.to_device(np.full(size, 0x4444, np.int16)), c.to_device(np.full(size, 0x6666, np.int16))
        assert c.L.vtmhip_lmcs_resi_batch_dev(c.h, d_org.ptr, d_pred.ptr, d_resi.ptr, d_dst.ptr, d_jobs.ptr, n) == lib.E_INVALID
        assert c.L.vtmhip_lmcs_reco_batch_dev(c.h, d_pred.ptr, d_rin.ptr, d_reco.ptr, d_jobs.ptr, n) == lib.E_INVALID
        assert (d_resi.to_host(np.int16) == 0x3333).all() and (d_reco.to_host(np.int16) == 0x6666).all()
        c.set_lmcs_fwd_lut(lut, bd)
        c.lmcs_resi_batch(d_org.ptr, d_pred.ptr, d_resi.ptr, d_jobs.ptr, n, d_dst.ptr)
        assert np.array_equal(d_resi.to_host(np.int16), exp_resi)
        assert np.array_equal(d_dst.to_host(np.int16), exp_dst)
        reco_jobs = (LmcsJob * (n // 2))(*[jobs[k] for k in range(n) if not specs[k][2] & lu.WRITE_MAPPED])
        c.lmcs_reco_batch(d_pred.ptr, d_rin.ptr, d_reco.ptr, c.to_device(np.frombuffer(reco_jobs, np.uint8)).ptr, n // 2)
        assert np.array_equal(d_reco.to_host(np.int16), exp_reco)
        # a sample outside the table is clamped into it, never read outside: org = -5 / 32767 map like 0 / top
        wild = np.array([-5, 32767, 3, top], np.int16)
        one = (LmcsJob * 1)()
        one[0].orgStride = one[0].predStride = one[0].resiStride = one[0].dstStride = 4
        one[0].width, one[0].height, one[0].bitDepth, one[0].flags = 4, 1, bd, 0
        d_out = c.to_device(np.zeros(4, np.int16))
        c.lmcs_resi_batch(c.to_device(wild).ptr, c.to_device(np.zeros(4, np.int16)).ptr, d_out.ptr, c.to_device(np.frombuffer(one, np.uint8)).ptr, 1)
        assert d_out.to_host(np.int16).tolist() == [int(lut[0]), int(lut[top]), int(lut[3]), int(lut[top])]


# ---- several jobs per wave ------------------------------------------------------------------------------------------------------------------------------
# The batch entries pack G = n / (32 * CUs) jobs per wave (at most 64).  n = 2 * 32 * CUs gives G = 2: the cursor over two jobs per wave, mixed shapes whose
# segment counts end inside a 64-segment step (the tall ones as the first and as the second job of a group), rejected jobs inside a group.
PACKED_SMALL, PACKED_TALL = [(1, 1), (2, 2), (4, 4), (8, 4), (3, 5)], [(4, 70), (12, 40), (6, 50)]   # tall: 70 / 120 / 100 row segments, no multiple of 64
_packed = {}


def _view(a, off, stride, w, h):
    return np.lib.stride_tricks.as_strided(a[off:], (h, w), (2 * stride, 2))


def _packed_specs(planes):
    """(n, [(w, h, tall, rejected, [(offset, stride)] * planes)], pool size): n = 2 * 32 * CUs jobs, ~6 % tall, every 97th rejected, odd strides and offsets"""
    if planes not in _packed:
        import torch
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        n = 2 * 32 * cus
        assert n // (32 * cus) == 2
        rng = np.random.default_rng(700 + planes)
        specs, cur = [], [0] * planes
        for k in range(n):
            tall = k % 32 in (3, 20)   # 20: the first job of its group of two, 3: the second
            w, h = PACKED_TALL[(k // 32) % 3] if tall else PACKED_SMALL[int(rng.integers(len(PACKED_SMALL)))]
            pl = []
            for b in range(planes):
                off, stride, cur[b] = _place(rng, cur[b], w, h)
                pl.append((off, stride))
            specs.append((w, h, tall, k % 97 == 96, pl))
        for first in (0, 1):
            assert sum(t and not rej for k, (_w, _h, t, rej, _pl) in enumerate(specs) if k % 2 == first) >= n // 40
        assert sum(rej for (_w, _h, _t, rej, _pl) in specs) == n // 97
        _packed[planes] = n, specs, max(cur) + 8
    return _packed[planes]


def _packed_luma(bd=10):
    n, specs, size = _packed_specs(4)
    rng = np.random.default_rng(710)
    top = (1 << bd) - 1
    return n, specs, size, lu.make_lut(77, bd), rng.integers(0, top + 1, size).astype(np.int16), rng.integers(0, top + 1, size).astype(np.int16), \
        rng.integers(-top, top + 1, size).astype(np.int16)


def test_lmcs_resi_with_several_jobs_per_wave(ctx, bd=10):
    """all four flag combinations; rejected inside groups: width 0, an unknown flag bit.  Outside the blocks and in a rejected job's block the sentinels stay."""
    n, specs, size, lut, org, pred, _rin = _packed_luma(bd)
    jobs = (LmcsJob * n)()
    exp_resi, exp_dst = np.full(size, 0x3333, np.int16), np.full(size, 0x4444, np.int16)
    for k, (w, h, _tall, rej, pl) in enumerate(specs):
        j, flags = jobs[k], (k // 2 + k) % 4
        (j.orgOff, j.orgStride), (j.predOff, j.predStride), (j.resiOff, j.resiStride), (j.dstOff, j.dstStride) = pl
        j.width, j.height, j.bitDepth, j.flags = w, h, bd, flags
        if rej:
            j.width, j.flags = (0, flags) if (k // 97) % 2 else (w, flags | 4)
            continue
        r, mapped = lu.resi_expect(_view(org, *pl[0], w, h), _view(pred, *pl[1], w, h), lut, flags & lu.MAP_PRED)
        _view(exp_resi, *pl[2], w, h)[:] = r
        if flags & lu.WRITE_MAPPED:
            _view(exp_dst, *pl[3], w, h)[:] = mapped
    assert {(j.flags, k % 2) for k, j in enumerate(jobs) if j.flags < 4} == {(f, p) for f in range(4) for p in range(2)}
    ctx.set_lmcs_fwd_lut(lut, bd)
    d_resi, d_dst = ctx.to_device(np.full(size, 0x3333, np.int16)), ctx.to_device(np.full(size, 0x4444, np.int16))
    bufs = [ctx.to_device(org), ctx.to_device(pred), ctx.to_device(np.frombuffer(jobs, np.uint8)), d_resi, d_dst]
    ctx.lmcs_resi_batch(bufs[0].ptr, bufs[1].ptr, d_resi.ptr, bufs[2].ptr, n, d_dst.ptr)
    assert np.array_equal(d_resi.to_host(np.int16), exp_resi)
    assert np.array_equal(d_dst.to_host(np.int16), exp_dst)
    for b in bufs:
        b.free()


def test_lmcs_reco_with_several_jobs_per_wave(ctx, bd=10):
    """both MAP_PRED settings; rejected inside groups: width 0, a flag bit the reconstruction does not know (WRITE_MAPPED, bit 2)"""
    n, specs, size, lut, _org, pred, rin = _packed_luma(bd)
    jobs = (LmcsJob * n)()
    exp = np.full(size, 0x6666, np.int16)
    for k, (w, h, _tall, rej, pl) in enumerate(specs):
        j, flags = jobs[k], ((k // 2 + k) % 2) * lu.MAP_PRED
        (j.predOff, j.predStride), (j.resiOff, j.resiStride), (j.dstOff, j.dstStride) = pl[1:]
        j.width, j.height, j.bitDepth, j.flags = w, h, bd, flags
        if rej:
            j.width, j.flags = [(0, flags), (w, flags | lu.WRITE_MAPPED), (w, flags | 4)][(k // 97) % 3]
            continue
        _view(exp, *pl[3], w, h)[:] = lu.reco_expect(_view(pred, *pl[1], w, h), _view(rin, *pl[2], w, h), lut, flags, bd)
    ctx.set_lmcs_fwd_lut(lut, bd)
    d_reco = ctx.to_device(np.full(size, 0x6666, np.int16))
    bufs = [ctx.to_device(pred), ctx.to_device(rin), ctx.to_device(np.frombuffer(jobs, np.uint8)), d_reco]
    ctx.lmcs_reco_batch(bufs[0].ptr, bufs[1].ptr, d_reco.ptr, bufs[2].ptr, n)
    assert np.array_equal(d_reco.to_host(np.int16), exp)
    for b in bufs:
        b.free()


def test_scale_signal_batch_with_several_jobs_per_wave(ctx):
    """both directions, the edge scales, 8 / 10 / 12 bits; rejected inside groups: scale 0, forward scaling of width 1 (a 1x1 block is otherwise scaled inversely)"""
    n, specs, size = _packed_specs(2)
    rng = np.random.default_rng(720)
    src, exp = rng.integers(-32768, 32768, size).astype(np.int16), np.full(size, 0x5555, np.int16)
    jobs = (ScaleJob * n)()
    for k, (w, h, _tall, rej, pl) in enumerate(specs):
        j = jobs[k]
        (j.srcOff, j.srcStride), (j.dstOff, j.dstStride) = pl
        scale, fwd, bd = lu.EDGE_SCALES[int(rng.integers(len(lu.EDGE_SCALES)))], (k // 2 + k) % 2 if w > 1 else 0, 8 + 2 * (k % 3)
        j.width, j.height, j.scale, j.dir, j.bitDepth = w, h, scale, fwd, bd
        if rej:
            if (k // 97) % 2:
                j.scale = 0
            else:
                j.width, j.dir = 1, 1
            continue
        _view(exp, *pl[1], w, h)[:] = lu.scale_signal(_view(src, *pl[0], w, h), scale, fwd, bd)
    bufs = [ctx.to_device(src), ctx.to_device(np.full(size, 0x5555, np.int16)), ctx.to_device(np.frombuffer(jobs, np.uint8))]
    ctx.scale_signal_batch(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, n)
    assert np.array_equal(bufs[1].to_host(np.int16), exp)
    for b in bufs:
        b.free()


# ---- the plain chain with CRS ------------------------------------------------------------------------------------------------------------------------
_tu, _jc = {}, {}
TU_SHAPES = {"generic": [(2, 2), (2, 4), (4, 2), (4, 16), (16, 4), (8, 8), (32, 32), (4, 4), (32, 32)],   # the last two: transform skip
             "lane": [(4, 4), (8, 4), (4, 8)],
             "blocked": [(8, 8), (16, 8), (8, 16), (32, 32)],
             "bucketed": [(8, 8), (16, 8), (16, 16), (4, 8)]}
TU_JOBS = {"generic": 90, "lane": 210, "blocked": 120, "bucketed": 320}


def _qp(rng, bd):
    q = int(rng.choice([22, 27, 32, 37])) + 6 * (bd - 8)
    return q // 6, q % 6


def _amp_adj(rng, k, bd):
    """amplitude and adj of job k: every third job drives fwd() into saturation and the reconstruction past the inverse's input clip (amplitude M, adj <= 512)"""
    m = (1 << bd) - 1
    if k % 3 == 0:
        return m, int(rng.choice([256, 300, 512]))
    return int(rng.choice([60, 400, m, m])), ADJS[int(rng.integers(0, len(ADJS)))]


def _tu_batch(kind, bd):
    if (kind, bd) not in _tu:
        rng = np.random.default_rng(2000 * bd + len(kind))
        shapes, specs = TU_SHAPES[kind], []
        for k in range(TU_JOBS[kind]):
            w, h = shapes[k % len(shapes)]
            ts = kind == "generic" and k % len(shapes) >= 7
            amp, adj = _amp_adj(rng, k // len(shapes) + k, bd)
            per, rem = _qp(rng, bd)
            specs.append((rng.integers(-amp, amp + 1, (h, w)).astype(np.int16), adj, per, rem, int(rng.integers(0, 2)), ts))
        if kind == "blocked":
            m = (1 << bd) - 1
            specs.append((rng.integers(-m, m + 1, (64, 64)).astype(np.int16), 300, (37 + 6 * (bd - 8)) // 6, (37 + 6 * (bd - 8)) % 6, 0, False))   # one 64x64
        _tu[(kind, bd)] = lu.TuBatch(specs, bd, col=5 if (kind, bd) == ("lane", 8) else 4)   # one lane batch on rows that are not 8-byte aligned
    return _tu[(kind, bd)]


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_tu_chain_crs_generic_path(ctx, bd):
    """One mixed launch on the LDS kernel: 2x2 with an adj set (the area rule: it equals the unscaled chain), 2x4 .. 32x32, transform skip 4x4 and 32x32."""
    b = _tu_batch("generic", bd)
    b.assert_bites()
    tiny = [k for k, s in enumerate(b.shapes) if s == (2, 2)]
    assert any(b.jobs[k].chromaAdj for k in tiny) and all(b.exp[k]["adj"] == 0 for k in tiny)
    assert sum(j.typeHor == lu.TRSKIP and j.chromaAdj > 0 for j in b.jobs) >= 8
    got = b.run(ctx, 32, 32)
    b.check(got)
    plain = b.run(ctx, 32, 32, idx=tiny, crs=False)
    assert lu.raw_results(plain[0], TU_FIELDS) == lu.raw_results([got[0][k] for k in tiny], TU_FIELDS)
    small = [k for k, (w, h) in enumerate(b.shapes) if w <= 16 and h <= 16]   # the 64-threads-per-TU variant of the same kernel
    b.check(b.run(ctx, 16, 16, idx=small), idx=small)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_tu_chain_crs_lane_path(ctx, bd):
    b = _tu_batch("lane", bd)
    b.assert_bites()
    for shape in TU_SHAPES["lane"]:
        idx = [k for k, s in enumerate(b.shapes) if s == shape]
        assert len(idx) > 64
        b.check(b.run(ctx, shape[0], shape[1], uniform=True, idx=idx), idx=idx)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_tu_chain_crs_blocked_path(ctx, bd):
    b = _tu_batch("blocked", bd)
    b.assert_bites()
    for shape in TU_SHAPES["blocked"] + [(64, 64)]:
        idx = [k for k, s in enumerate(b.shapes) if s == shape]
        idx = idx[:-1] if len(idx) > 1 else idx      # 29 jobs: the last workgroup is not full
        b.check(b.run(ctx, shape[0], shape[1], uniform=True, idx=idx), idx=idx)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_tu_chain_crs_bucketed_path(ctx, bd):
    """320 mixed jobs, a different adj per job and some 0, in one non-uniform launch: bucketed by shape on the device, every result back at its own index."""
    b = _tu_batch("bucketed", bd)
    b.assert_bites()
    adjs = [j.chromaAdj for j in b.jobs]
    assert b.n == 320 and len(set(adjs)) >= 8 and adjs.count(0) >= 10
    order = [int(k) for k in np.random.default_rng(bd).permutation(b.n)]
    ctx.kernel_timing(True)
    try:
        got = b.run(ctx, 16, 16, idx=order)
        launches = [ctx.kernel_timing_read(k)[1] for k in ("tu_chain_uni_kernel", "tu_chain_kernel")]
    finally:
        ctx.kernel_timing(False)
    b.check(got, idx=order)
    assert launches[0] == 3, launches     # the three classes with sides >= 8 went to the register-blocked kernel: the batch was bucketed


# ---- the joint chain with CRS ------------------------------------------------------------------------------------------------------------------------
JC_SHAPES = {"generic": [(2, 2), (2, 8), (4, 4), (8, 4), (16, 4), (8, 8), (16, 16), (32, 32)], "lane": [(4, 4), (8, 4), (4, 8)], "blocked": [(8, 8), (16, 16), (32, 8), (32, 32)]}
JC_JOBS = {"generic": 96, "lane": 216, "blocked": 96}


def _jc_batch(kind, bd):
    if (kind, bd) not in _jc:
        rng = np.random.default_rng(3000 * bd + len(kind))
        shapes, specs = JC_SHAPES[kind], []
        for k in range(JC_JOBS[kind]):
            w, h = shapes[k % len(shapes)]
            mode = SIGNED_MODES[(k // len(shapes)) % 6]
            amp, adj = _amp_adj(rng, k // len(shapes) + k, bd)
            cb, cr = ju.recipe_pair(rng, w, h, bd, amp, mode)
            per, rem = _qp(rng, bd)
            ts = kind == "generic" and (k + k // len(shapes)) % 4 == 3 and w * h > 4
            specs.append((cb, cr, adj, ju.mask_of(mode), int(mode < 0), per, rem, int(rng.integers(0, 2)), ts))
        _jc[(kind, bd)] = lu.JccrBatch(specs, bd, cb_col=5 if (kind, bd) == ("lane", 8) else 4)
    return _jc[(kind, bd)]


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_jccr_chain_crs_generic_path(ctx, bd):
    b = _jc_batch("generic", bd)
    b.assert_bites()
    assert {ju.mode_of(j.signFlag, j.cbfMask) for j in b.jobs} == set(SIGNED_MODES)
    assert sum(j.typeHor == lu.TRSKIP and j.chromaAdj > 0 for j in b.jobs) >= 8
    b.check(b.run(ctx, 32, 32))
    small = [k for k, (w, h) in enumerate(b.shapes) if w <= 16 and h <= 16]
    b.check(b.run(ctx, 16, 16, idx=small), idx=small)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_jccr_chain_crs_lane_path(ctx, bd):
    b = _jc_batch("lane", bd)
    b.assert_bites()
    for shape in JC_SHAPES["lane"]:
        idx = [k for k, s in enumerate(b.shapes) if s == shape]
        assert len(idx) > 64 and {ju.mode_of(b.jobs[k].signFlag, b.jobs[k].cbfMask) for k in idx} == set(SIGNED_MODES)
        b.check(b.run(ctx, shape[0], shape[1], uniform=True, idx=idx), idx=idx)


@pytest.mark.parametrize("bd", [8, 10, 12])
def test_jccr_chain_crs_blocked_path(ctx, bd):
    b = _jc_batch("blocked", bd)
    b.assert_bites()
    for shape in JC_SHAPES["blocked"]:
        idx = [k for k, s in enumerate(b.shapes) if s == shape][:-1]   # 23 jobs: the last workgroup is not full
        assert {ju.mode_of(b.jobs[k].signFlag, b.jobs[k].cbfMask) for k in idx} == set(SIGNED_MODES)
        b.check(b.run(ctx, shape[0], shape[1], uniform=True, idx=idx), idx=idx)


# ---- equivalences and argument errors ---------------------------------------------------------------------------------------------------------------
def _same(a, b, fields):
    assert lu.raw_results(a[0], fields) == lu.raw_results(b[0], fields)
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("kind", ["generic", "lane", "blocked", "bucketed"])
def test_tu_chain_equivalences(ctx, kind, bd=10):
    """The CRS entry with every adj 0 is the plain entry, field for field; the plain entry ignores an adj in the bytes that were its padding."""
    b = _tu_batch(kind, bd)
    assert sum(j.chromaAdj != 0 for j in b.jobs) * 2 > b.n
    runs = [(16, 16, False, None)] if kind == "bucketed" else [(32, 32, False, [k for k, s in enumerate(b.shapes) if s != (64, 64)])] if kind == "generic" else \
        [(w, h, True, [k for k, s in enumerate(b.shapes) if s == (w, h)]) for (w, h) in TU_SHAPES[kind]]
    for (mw, mh, uni, idx) in runs:
        plain = b.run(ctx, mw, mh, uniform=uni, idx=idx, crs=False, adj_override=0)
        _same(b.run(ctx, mw, mh, uniform=uni, idx=idx, crs=True, adj_override=0), plain, TU_FIELDS)
        _same(b.run(ctx, mw, mh, uniform=uni, idx=idx, crs=False), plain, TU_FIELDS)
        assert any(r.absSum > 0 for r in plain[0])


@pytest.mark.parametrize("kind", ["generic", "lane", "blocked"])
def test_jccr_chain_equivalences(ctx, kind, bd=10):
    b = _jc_batch(kind, bd)
    assert sum(j.chromaAdj != 0 for j in b.jobs) * 2 > b.n
    runs = [(32, 32, False, None)] if kind == "generic" else [(w, h, True, [k for k, s in enumerate(b.shapes) if s == (w, h)]) for (w, h) in JC_SHAPES[kind]]
    for (mw, mh, uni, idx) in runs:
        plain = b.run(ctx, mw, mh, uniform=uni, idx=idx, crs=False, adj_override=0)
        _same(b.run(ctx, mw, mh, uniform=uni, idx=idx, crs=True, adj_override=0), plain, JC_FIELDS)
        _same(b.run(ctx, mw, mh, uniform=uni, idx=idx, crs=False), plain, JC_FIELDS)
        assert any(r.absSum > 0 for r in plain[0])


def test_plain_chain_treats_an_out_of_range_adj_as_zero(ctx, bd=10):
    """The plain chain's table stays on the device: an adj outside 0 .. 32767 is documented to count as 0."""
    b = _tu_batch("lane", bd)
    idx = [k for k, s in enumerate(b.shapes) if s == (4, 4)]
    zero = b.run(ctx, 4, 4, uniform=True, idx=idx, adj_override=0)
    for adj in (40000, -1, 32768):
        _same(b.run(ctx, 4, 4, uniform=True, idx=idx, adj_override=adj), zero, TU_FIELDS)


def test_crs_argument_errors_launch_nothing(ctx):
    """An adj of 40000 on the joint chain, and the plain joint entry's own checks through the CRS entry, return VTMHIP_E_INVALID and launch no kernel."""
    resi = np.zeros((64, 160), np.int16)

    def call(adj, mask=3, w=8, h=8, type_hor=0, n=2, uniform=False, max_wh=(64, 64)):
        jobs = (JccrJob * 2)()
        for k in range(2):
            j = jobs[k]
            j.cbOff, j.crOff, j.resiStride, j.outOff, j.width, j.height = 0, 80, 160, k * 4096, 8, 8
            j.qpPer, j.qpRem, j.typeHor, j.bitDepth, j.isIRAP, j.cbfMask, j.signFlag, j.chromaAdj = 5, 2, 0, 10, 0, 3, 0, 2048
        j = jobs[1]
        j.cbfMask, j.width, j.height, j.typeHor, j.chromaAdj = mask, w, h, type_hor, adj
        d_resi, d_jobs = ctx.to_device(resi), ctx.to_device(np.frombuffer(jobs, np.uint8))
        d_res = ctx.to_device(np.full(2 * C.sizeof(JccrResult), 0xA5, np.uint8))
        ctx.kernel_timing(True)
        try:
            st = ctx.L.vtmhip_jccr_chain_crs_batch_dev(ctx.h, d_resi.ptr, d_jobs.ptr, n, max_wh[0], max_wh[1], int(uniform), None, None, None, d_res.ptr)
            launches = sum(ctx.kernel_timing_read(k)[1] for k in ("jccr_chain_kernel", "jccr_chain_lane_kernel", "jccr_chain_uni_kernel"))
        finally:
            ctx.kernel_timing(False)
        return st, launches, bool((d_res.to_host(np.uint8) == 0xA5).all())

    assert call(32767) == (lib.OK, 1, False)
    assert call(0) == (lib.OK, 1, False)
    assert call(40000) == (lib.E_INVALID, 0, True)
    assert call(32768) == (lib.E_INVALID, 0, True)
    assert call(2048, mask=0) == (lib.E_INVALID, 0, True)
    assert call(2048, mask=4) == (lib.E_INVALID, 0, True)
    assert call(2048, w=64, h=8, type_hor=ju.TRSKIP) == (lib.E_INVALID, 0, True)
    assert call(2048, type_hor=1) == (lib.E_INVALID, 0, True)
    assert call(2048, w=16, h=16, uniform=True, max_wh=(8, 8)) == (lib.E_INVALID, 0, True)
    assert call(40000, n=0) == (lib.OK, 0, True)
    assert ctx.L.vtmhip_jccr_chain_crs_batch_dev(ctx.h, None, None, 2, 64, 64, 0, None, None, None, None) == lib.E_INVALID
    assert ctx.L.vtmhip_tu_chain_crs_batch_dev(ctx.h, None, None, 2, 64, 64, 0, None, None, None) == lib.E_INVALID
    assert ctx.L.vtmhip_tu_chain_crs_batch_dev(ctx.h, None, None, 0, 64, 64, 0, None, None, None) == lib.OK
    assert C.sizeof(TuResult) == 16
