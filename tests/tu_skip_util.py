"""For tests/test_gpu_tu_zero_skip.py: TUs with their expectations from the oracle's separate steps (formed as
tests/test_gpu_transform.py::test_tu_chain_matches_oracle forms them: vo_fwd_2d, vo_quant, vo_dequant, vo_inv_2d, o_dist), and one launch of the fused chain
compared against them in full -- sse, sumAbs, absSum, every level, every reconstructed sample -- once into sentinel-filled buffers and once without them."""
import ctypes as C

import numpy as np

import lmcs_util as lu
import oracle_lib as ol

MTS_PAIRS = [(0, 0), (2, 2), (1, 2), (2, 1), (1, 1)]   # (typeHor, typeVer): DCT-2, then the DST-7 / DCT-8 pairs of the MTS candidates
SENTINEL = -7


def qp_of(qp, bd):
    """(qpPer, qpRem) of a QP at a bit depth, as the driver passes them"""
    q = qp + 6 * (bd - 8)
    return q // 6, q % 6


def types_of(w, h, k):
    return MTS_PAIRS[k % len(MTS_PAIRS)] if max(w, h) <= 32 else (0, 0)


class Tu:
    """One TU: its residual block and job fields, and what the chain must return for it."""

    def __init__(self, blk, bd, qp, th=0, tv=0, irap=0, adj=0):
        L = ol.oracle()
        self.blk = np.ascontiguousarray(blk, np.int16)
        h, w = self.blk.shape
        self.w, self.h, self.bd, self.th, self.tv, self.irap, self.adj = w, h, bd, th, tv, irap, adj
        self.per, self.rem = qp_of(qp, bd)
        if adj:
            assert (th, tv) == (0, 0)
            e = lu.tu_chain_expect(self.blk, adj, bd, self.per, self.rem, irap, 0)
            self.sse, self.sumAbs, self.absSum, self.levels, self.rec = e["sse"], e["sumAbs"], e["absSum"], e["levels"], e["rec"]
            return
        coef, qc, dq = np.zeros(w * h, np.int32), np.zeros(w * h, np.int32), np.zeros(w * h, np.int32)
        assert L.vo_fwd_2d(ol.P(self.blk), w, w, h, bd, th, tv, ol.P(coef)) == 0
        s = C.c_int32()
        L.vo_quant(ol.P(coef), w, h, bd, self.per, self.rem, irap, 0, ol.P(qc), None, C.byref(s))
        L.vo_dequant(ol.P(qc), w, h, bd, self.per, self.rem, 0, ol.P(dq))
        rec = np.zeros((h, w), np.int16)
        assert L.vo_inv_2d(ol.P(dq), w, h, bd, th, tv, ol.P(rec), w) == 0
        self.sse, self.sumAbs, self.absSum = int(ol.o_dist(2, self.blk, rec, w, h)), int(np.abs(coef.astype(np.int64)).sum()), s.value
        self.levels, self.rec = qc, rec.reshape(-1)


def run_check(ctx, tus, max_w, max_h, uniform, crs=False, tag=None):
    """One launch over `tus` (in this order), with levels / rec buffers full of a sentinel, then the same launch without them."""
    from vtm_amd.lib import TuJob, TuResult
    n, rows, stride, slot = len(tus), max(t.h for t in tus), max(t.w for t in tus) + 8, max(t.w * t.h for t in tus)
    resi = np.full((n * rows, stride), 77, np.int16)   # the samples around a block are not zero
    jobs = (TuJob * n)()
    for k, t in enumerate(tus):
        resi[k * rows:k * rows + t.h, 4:4 + t.w] = t.blk
        j = jobs[k]
        j.resiOff, j.outOff, j.resiStride, j.width, j.height = k * rows * stride + 4, k * slot, stride, t.w, t.h
        j.qpPer, j.qpRem, j.typeHor, j.typeVer, j.bitDepth, j.isIRAP, j.chromaAdj = t.per, t.rem, t.th, t.tv, t.bd, t.irap, t.adj
    d_resi, d_jobs = ctx.to_device(resi), ctx.to_device(np.frombuffer(jobs, np.uint8))
    fn = ctx.tu_chain_crs_batch if crs else ctx.tu_chain_batch
    exp = [(t.sse, t.sumAbs, t.absSum) for t in tus]
    for with_out in (True, False):
        d_res = ctx.to_device(np.full(C.sizeof(TuResult) * n, 0xA5, np.uint8))
        d_lv, d_rec = ctx.to_device(np.full((n, slot), SENTINEL, np.int32)), ctx.to_device(np.full((n, slot), SENTINEL, np.int16))
        fn(d_resi.ptr, d_jobs.ptr, n, max_w, max_h, d_res.ptr, d_lv.ptr if with_out else None, d_rec.ptr if with_out else None, uniform=uniform)
        res = (TuResult * n).from_buffer_copy(d_res.to_host(np.uint8).tobytes())
        got = [(r.sse, r.sumAbs, r.absSum) for r in res]
        lv, rc = d_lv.to_host().reshape(n, slot), d_rec.to_host().reshape(n, slot)
        for d in (d_res, d_lv, d_rec):
            d.free()
        bad = [k for k in range(n) if got[k] != exp[k]]
        assert not bad, (tag, with_out, [(k, tus[k].w, tus[k].h, tus[k].th, tus[k].tv, got[k], exp[k]) for k in bad[:6]])
        for k, t in enumerate(tus):
            m = t.w * t.h
            if with_out:
                assert np.array_equal(lv[k, :m], t.levels), (tag, "levels", k, t.w, t.h)
                assert np.array_equal(rc[k, :m], t.rec), (tag, "rec", k, t.w, t.h)
                assert (lv[k, m:] == SENTINEL).all() and (rc[k, m:] == SENTINEL).all(), (tag, "wrote past its slot", k)
            else:
                assert (lv[k] == SENTINEL).all() and (rc[k] == SENTINEL).all(), (tag, "wrote to a buffer it was not given", k)
    d_resi.free()
    d_jobs.free()
