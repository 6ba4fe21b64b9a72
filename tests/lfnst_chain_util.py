"""Tables and expectations of the LFNST residual chain (vtmhip_lfnst_chain_batch_dev, vtmhip_intra_chain_lfnst_batch_dev) for the CPU and GPU tests.

Two expectations of one job.  oracle_chain: no device entry at all -- the CPU oracle's vo_fwd_trans / vo_inv_trans with the LFNST skips, vo_lfnst_tu, vo_quant and
vo_dequant, numpy between them.  device_chain: the pinned device entries xT -> forward LFNST -> quant -> dequant -> inverse LFNST -> xIT with numpy zeroing outside the
kept region and outside the coded scan positions; it rests on the fact that zero-out only omits coefficients and never changes the kept ones.
An LfnstLevel is an intra_chain_util.Level with a second candidate table: (pred, qp, irap, lfnstIdx) per LFNST job."""
import ctypes as C
import os

import numpy as np

import intra_chain_util as icu
import oracle_lib as ol
from vtm_amd import lib
from vtm_amd.lib import IntraLfnstTuJob, LfnstChainJob, LfnstTuJob, QuantJob, TrJob

GAP, FILL, FILL16, FILL32 = icu.GAP, icu.FILL, icu.FILL16, icu.FILL32
RES_DT = np.dtype([("sse", "<u8"), ("sumAbs", "<i4"), ("absSum", "<i4")])
IRES_DT = np.dtype([("sse", "<u8"), ("sseResi", "<u8"), ("sumAbs", "<i4"), ("absSum", "<i4")])
_mats = None


def matrices():
    """(g_lfnst8x8 [4][2][16][48], g_lfnst4x4 [4][2][16][16]): the golden copy of the reference's tables"""
    global _mats
    if _mats is None:
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lfnst.npz"))
        _mats = np.ascontiguousarray(z["m8"]), np.ascontiguousarray(z["m4"])
    return _mats


def keep_of(w, h):
    return 8 if (w >= 8 and h >= 8) else 4


def zero_out_of(w, h):
    return 8 if (w, h) in ((4, 4), (8, 8)) else 16


def coded_positions(w, h):
    pos = np.zeros(48, np.int32)
    ol.oracle().vo_lfnst_scan(w, h, ol.P(pos))
    return pos[:zero_out_of(w, h)]


def core_matrix(w, h, set_idx, index):
    m8, m4 = matrices()
    return np.ascontiguousarray((m8 if (w >= 8 and h >= 8) else m4)[set_idx, index])


def mode_of(w, h, mode, is_mip):
    """the Python restatement of the mode rule: PU::getWideAngle, getLFNSTIntraMode, the set ranges of H.266 8.7.4.1, getTransposeFlag"""
    wide = 0 if is_mip else mode
    if not is_mip and mode > 1:
        shift = [0, 6, 10, 12, 14, 15][abs(w.bit_length() - h.bit_length())]
        if w > h and mode < 2 + shift:
            wide = mode + 65
        elif h > w and mode > 66 - shift:
            wide = mode - 67
    intra = wide + 81 if wide < 0 else wide + 14 if wide >= 67 else wide
    set_idx = 1 if wide < 0 else 0 if wide <= 1 else 1 if wide <= 12 else 2 if wide <= 23 else 3 if wide <= 44 else 2 if wide <= 55 else 1
    return set_idx, int(intra >= 81 if intra >= 67 else intra > 34)


def oracle_chain(resi, w, h, bd, per, rem, irap, set_idx, index, transpose):
    """resi: [h, w] int16 -> dict(levels [w * h] int32, rec [h, w] int16, result (sse, sumAbs, absSum), dropped: the primary coefficients Quant::quant never reads)"""
    L = ol.oracle()
    keep, lw, lh = keep_of(w, h), w.bit_length() - 1, h.bit_length() - 1
    block = np.ascontiguousarray(resi, np.int32).reshape(-1)
    tmp, coef = np.zeros(w * h, np.int32), np.zeros(w * h, np.int32)
    assert L.vo_fwd_trans(0, w, ol.P(block), ol.P(tmp), lw + bd + 6 - 15, h, 0, w - keep) == 0
    assert L.vo_fwd_trans(0, h, ol.P(tmp), ol.P(coef), lh + 6, w, w - keep, h - keep) == 0
    M = core_matrix(w, h, set_idx, index)
    L.vo_lfnst_tu(ol.P(coef), w, h, ol.P(M), transpose, 0)
    pos = coded_positions(w, h)
    kept = np.zeros(w * h, np.int32)
    kept[pos] = coef[pos]
    dropped = coef.copy()
    dropped[pos] = 0
    qc, dq, s = np.zeros(w * h, np.int32), np.zeros(w * h, np.int32), C.c_int32()
    L.vo_quant(ol.P(kept), w, h, bd, per, rem, irap, 0, ol.P(qc), None, C.byref(s))
    L.vo_dequant(ol.P(qc), w, h, bd, per, rem, 0, ol.P(dq))
    L.vo_lfnst_tu(ol.P(dq), w, h, ol.P(M), transpose, 1)
    out = np.zeros(w * h, np.int32)
    assert L.vo_inv_trans(0, h, ol.P(dq), ol.P(tmp), 7, w, w - keep, h - keep, -32768, 32767) == 0
    assert L.vo_inv_trans(0, w, ol.P(tmp), ol.P(out), 20 - bd, h, 0, w - keep, -32768, 32767) == 0
    rec = out.astype(np.int16).reshape(h, w)
    d = np.asarray(resi, np.int64) - rec
    return dict(levels=qc, rec=rec, result=(int((d * d).sum()), int(np.abs(kept.astype(np.int64)).sum()), s.value), dropped=dropped)


def chain_job(resi_off, out_off, stride, w, h, bd, per, rem, irap, set_idx, index, transpose):
    return LfnstChainJob(resi_off, out_off, stride, w, h, per, rem, bd, irap, set_idx, index, transpose)


def device_chain(ctx, resi_buf, jobs):
    """the composition of pinned device entries over a whole LfnstChainJob table -> (levels per job, rec per job [h, w], (sse, sumAbs, absSum) per job)"""
    from vtm_amd.device import struct_array_to_numpy as s2n
    n, area = len(jobs), 4096
    tr, ltu, qj = (TrJob * n)(), (LfnstTuJob * n)(), (QuantJob * n)()
    for k, j in enumerate(jobs):
        tr[k] = TrJob(j.resiOff, k * area, j.resiStride, j.width, j.width, j.height, lib.DCT2, lib.DCT2, j.bitDepth, 0)
        ltu[k] = LfnstTuJob(k * area, j.width, j.height, j.setIdx, j.index, j.transpose, 0)
        qj[k] = QuantJob(k * area, k * area, j.width, j.height, j.qpPer, j.qpRem, j.bitDepth, j.isIRAP, 0, 0, 0)
    mw, mh = max(j.width for j in jobs), max(j.height for j in jobs)
    d_resi, d_coef, d_tr = ctx.to_device(resi_buf), ctx.to_device(np.zeros(n * area, np.int32)), ctx.to_device(s2n(tr))
    ctx.xT_batch(d_resi.ptr, d_coef.ptr, d_tr.ptr, n, mw, mh)
    ctx.sync()
    coef = d_coef.to_host(np.int32, shape=(-1,)).copy()
    for k, j in enumerate(jobs):                                   # zero outside the kept region
        w, h, kp = j.width, j.height, keep_of(j.width, j.height)
        blk = coef[k * area:k * area + w * h].reshape(h, w)
        blk[kp:, :] = 0
        blk[:, kp:] = 0
    d_c2, d_ltu = ctx.to_device(coef), ctx.to_device(s2n(ltu))
    ctx.lfnst_tu_batch(d_c2.ptr, d_ltu.ptr, n)
    ctx.sync()
    coef = d_c2.to_host(np.int32, shape=(-1,)).copy()
    sum_abs = []
    for k, j in enumerate(jobs):                                   # zero outside the coded scan positions
        w, h = j.width, j.height
        pos, blk = coded_positions(w, h), coef[k * area:k * area + w * h]
        kept = np.zeros(w * h, np.int32)
        kept[pos] = blk[pos]
        blk[:] = kept
        sum_abs.append(int(np.abs(kept.astype(np.int64)).sum()))
    d_c3, d_q, d_qj, d_abs = ctx.to_device(coef), ctx.to_device(np.zeros(n * area, np.int32)), ctx.to_device(s2n(qj)), ctx.alloc(4 * n)
    ctx.quant_batch(d_c3.ptr, d_q.ptr, None, d_qj.ptr, n, d_abs.ptr)
    d_dq = ctx.to_device(np.zeros(n * area, np.int32))
    ctx.dequant_batch(d_q.ptr, d_dq.ptr, d_qj.ptr, n)
    for k in range(n):
        ltu[k].inverse = 1
    d_ltu2 = ctx.to_device(s2n(ltu))
    ctx.lfnst_tu_batch(d_dq.ptr, d_ltu2.ptr, n)
    for k, j in enumerate(jobs):
        tr[k] = TrJob(k * area, k * area, j.width, j.width, j.width, j.height, lib.DCT2, lib.DCT2, j.bitDepth, 0)
    d_tr2, d_rec = ctx.to_device(s2n(tr)), ctx.to_device(np.zeros(n * area, np.int16))
    ctx.xIT_batch(d_dq.ptr, d_rec.ptr, d_tr2.ptr, n, mw, mh)
    ctx.sync()
    q, rec, abs_sum = d_q.to_host(np.int32, shape=(-1,)), d_rec.to_host(np.int16, shape=(-1,)), d_abs.to_host(np.int32, shape=(-1,))
    levels, recs, results = [], [], []
    for k, j in enumerate(jobs):
        w, h = j.width, j.height
        levels.append(q[k * area:k * area + w * h].copy())
        r = rec[k * area:k * area + w * h].reshape(h, w).copy()
        recs.append(r)
        src = np.array([resi_buf[j.resiOff + y * j.resiStride:j.resiOff + y * j.resiStride + w] for y in range(h)], np.int64)
        d = src - r
        results.append((int((d * d).sum()), sum_abs[k], int(abs_sum[k])))
    for b in (d_resi, d_coef, d_tr, d_c2, d_ltu, d_c3, d_q, d_qj, d_abs, d_dq, d_ltu2, d_tr2, d_rec):
        b.free()
    return levels, recs, results


class ChainTable:
    """jobs of vtmhip_lfnst_chain_batch_dev over residual blocks at odd offsets with a stride above W, outputs between GAP samples of fill.
    specs: (w, h, bd, qp, irap, setIdx, index, transpose, resi [h, w] int16)"""
    def __init__(self, specs, order=None):
        specs = [specs[k] for k in order] if order is not None else list(specs)
        self.specs, parts, off, out = specs, [np.full(7, FILL16, np.int16)], 7, GAP
        jobs = []
        for w, h, bd, qp, irap, s, i, t, resi in specs:
            stride = w + 3
            buf = np.full(h * stride + 1, FILL16, np.int16)
            for y in range(h):
                buf[y * stride:y * stride + w] = resi[y]
            per, rem = icu.qp_of(qp, bd)
            jobs.append(chain_job(off, out, stride, w, h, bd, per, rem, irap, s, i, t))
            parts.append(buf)
            off += buf.size
            out += w * h + GAP
        self.resi_buf, self.out_len, self.n = np.concatenate(parts), out, len(specs)
        self.jobs = (LfnstChainJob * max(self.n, 1))(*jobs)

    def oracle(self):
        return [oracle_chain(sp[8], sp[0], sp[1], sp[2], self.jobs[k].qpPer, self.jobs[k].qpRem, sp[4], sp[5], sp[6], sp[7]) for k, sp in enumerate(self.specs)]

    def run(self, ctx, levels=True, rec=True, n=None):
        from vtm_amd.device import struct_array_to_numpy as s2n
        n = self.n if n is None else n
        ins = [ctx.to_device(self.resi_buf), ctx.to_device(s2n(self.jobs))]
        outs = [ctx.to_device(np.full(k, FILL, np.uint8)) for k in (4 * self.out_len, 2 * self.out_len, 16 * max(self.n, 1))]
        status = lib.OK
        try:
            ctx.lfnst_chain_batch(ins[0].ptr, ins[1].ptr, n, outs[2].ptr, outs[0].ptr if levels else None, outs[1].ptr if rec else None)
        except lib.VtmHipError as e:
            status = e.status
        ctx.sync()
        got = dict(status=status, levels=outs[0].to_host(np.int32, shape=(-1,)), rec=outs[1].to_host(np.int16, shape=(-1,)),
                   results=np.frombuffer(outs[2].to_host(np.uint8, shape=(-1,)).tobytes(), RES_DT))
        for b in ins + outs:
            b.free()
        return got

    def expected_buffers(self, per_job):
        """per_job: (levels, rec [h, w], result) per job -> the three output buffers in full"""
        levels, rec = np.full(self.out_len, FILL32, np.int32), np.full(self.out_len, FILL16, np.int16)
        for k, (lv, r, _) in enumerate(per_job):
            o, n = self.jobs[k].outOff, lv.size
            levels[o:o + n], rec[o:o + n] = lv, r.reshape(-1)
        return levels, rec, [tuple(p[2]) for p in per_job]

    def check(self, got, per_job, levels=True, rec=True):
        el, er, res = self.expected_buffers(per_job)
        assert got["status"] == lib.OK
        assert np.array_equal(got["levels"], el if levels else np.full(self.out_len, FILL32, np.int32)), np.argwhere(got["levels"] != el)[:6].tolist()
        assert np.array_equal(got["rec"], er if rec else np.full(self.out_len, FILL16, np.int16)), np.argwhere(got["rec"] != er)[:6].tolist()
        g = [tuple(int(v) for v in r) for r in got["results"][:self.n]]
        assert g == res, [(k, a, b) for k, (a, b) in enumerate(zip(g, res)) if a != b][:4]

    def untouched(self, got):
        return all((got[k].view(np.uint8) == FILL).all() for k in ("levels", "rec", "results"))


# ---- the level entry ---------------------------------------------------------------------------------------------------------------------------------------------
def expand(blocks, intra_jobs, n_intra, mip_jobs, lfnst_jobs):
    """the Python restatement of the LFNST half of vtmhip_intra_chain_lfnst_make_jobs: [dict of every vtmhip_lfnst_chain_job field], lanes per job"""
    out, area = [], 0
    for t in lfnst_jobs:
        is_mip = t.pred >= n_intra
        j = mip_jobs[t.pred - n_intra] if is_mip else intra_jobs[t.pred]
        b = blocks[j.block]
        s, tr = mode_of(b.width, b.height, j.mode, is_mip)
        out.append(dict(resiOff=j.predOff, outOff=t.outOff, resiStride=b.width, width=b.width, height=b.height, qpPer=t.qpPer, qpRem=t.qpRem, bitDepth=b.bitDepth,
                        isIRAP=t.isIRAP, setIdx=s, index=t.lfnstIdx - 1, transpose=tr, pad=[0] * 7))
        area = max(area, b.width * b.height)
    return out, (0 if not out else 16 if area <= 256 else 64)


def chain_fields(j):
    return {f: (list(getattr(j, f)) if f == "pad" else getattr(j, f)) for f, _ in LfnstChainJob._fields_}


class LfnstLevel(icu.Level):
    """lfnst: (pred, qp, irap, lfnstIdx) per LFNST job; their outputs follow the plain jobs' in the levels / reconstruction buffers"""
    def __init__(self, blocks, plane, tus, lfnst, order=None, lfnst_order=None):
        super().__init__(blocks, plane, tus, order)
        lfnst = [lfnst[k] for k in lfnst_order] if lfnst_order is not None else list(lfnst)
        self.lfnst, off, arr = lfnst, self.out_len, []
        for p, qp, irap, idx in lfnst:
            b = blocks[self.preds[p][0]]
            per, rem = icu.qp_of(qp, b["bd"])
            arr.append(IntraLfnstTuJob(off, p, per, rem, idx, irap))
            off += b["w"] * b["h"] + GAP
        self.out_len, self.n_lf = off, len(lfnst)
        self.lf_arr = (IntraLfnstTuJob * max(self.n_lf, 1))(*arr)
        self._lexp = None

    def host_jobs(self):
        """vtmhip_intra_chain_lfnst_make_jobs over the five tables: (TuJob array, LfnstChainJob array, maxWidth, maxHeight, uniform, lanes per LFNST job)"""
        from vtm_amd.device import intra_chain_lfnst_make_jobs
        return intra_chain_lfnst_make_jobs(self.blk_arr if self.blocks else None, self.intra_arr if self.n_intra else None, self.mip_arr if self.n_mip else None,
                                           self.tu_arr if self.n_tu else None, self.lf_arr if self.n_lf else None)

    def block_of_lf(self, k):
        return self.blocks[self.preds[self.lf_arr[k].pred][0]]

    def mode_of_lf(self, k):
        p, b = self.lf_arr[k].pred, self.block_of_lf(k)
        return mode_of(b["w"], b["h"], 0 if p >= self.n_intra else self.ij[p][1], p >= self.n_intra)

    def lf_device_args(self, ctx, levels=True, n_tu=None, n_lf=None):
        """(the arguments of Context.intra_chain_lfnst_batch in order, inputs, outputs): ref, org, blocks, numBlocks, intra jobs, nIntra, MIP jobs, nMip, TU jobs, nTu,
        LFNST jobs, nLfnst, pred, resi, reco, results, LFNST results, levels"""
        from vtm_amd.device import struct_array_to_numpy as s2n
        a, ins, outs = self.device_args(ctx, levels, n_tu)
        d_lf, d_lres = ctx.to_device(s2n(self.lf_arr)), ctx.to_device(np.full(24 * max(self.n_lf, 1), FILL, np.uint8))
        args = a[:10] + [d_lf.ptr, self.n_lf if n_lf is None else n_lf] + a[10:14] + [d_lres.ptr, a[14]]
        return args, ins + [d_lf], outs + [d_lres]

    def run_lf(self, ctx, levels=True, n_tu=None, n_lf=None):
        args, ins, outs = self.lf_device_args(ctx, levels, n_tu, n_lf)
        status = lib.OK
        try:
            ctx.intra_chain_lfnst_batch(*args)
        except lib.VtmHipError as e:
            status = e.status
        ctx.sync()
        got = dict(status=status, pred=outs[0].to_host(np.int16, shape=(-1,)), resi=outs[1].to_host(np.int16, shape=(-1,)), levels=outs[2].to_host(np.int32, shape=(-1,)),
                   reco=outs[3].to_host(np.int16, shape=(-1,)), results=np.frombuffer(outs[4].to_host(np.uint8, shape=(-1,)).tobytes(), IRES_DT),
                   lf_results=np.frombuffer(outs[5].to_host(np.uint8, shape=(-1,)).tobytes(), IRES_DT))
        for b in ins + outs:
            b.free()
        return got

    def lf_job_expect(self, k, pred, resi):
        """LFNST job k from its prediction and residual ([h, w]) and the oracle chain: dict(levels, reco, raw, result (sse, sseResi, sumAbs, absSum))"""
        t, b = self.lf_arr[k], self.block_of_lf(k)
        s, tr = self.mode_of_lf(k)
        e = oracle_chain(resi, b["w"], b["h"], b["bd"], t.qpPer, t.qpRem, t.isIRAP, s, t.lfnstIdx - 1, tr)
        raw = pred.astype(np.int64) + e["rec"]
        reco = np.clip(raw, 0, (1 << b["bd"]) - 1)
        d = self.org_of(b) - reco
        return dict(levels=e["levels"], reco=reco.reshape(-1).astype(np.int16), raw=raw, result=(int((d * d).sum()),) + e["result"])

    def lf_expect(self, ctx):
        """the plain half as Level.expect composes it, the LFNST half from the same predictions and residuals through the oracle chain"""
        if self._lexp is not None:
            return self._lexp
        base_len, self.out_len = self.out_len, self.lf_arr[0].outOff if self.n_lf else self.out_len
        try:
            exp = dict(self.expect(ctx))
        finally:
            self.out_len = base_len
        levels, reco = np.full(self.out_len, FILL32, np.int32), np.full(self.out_len, FILL16, np.int16)
        levels[:exp["levels"].size], reco[:exp["reco"].size] = exp["levels"], exp["reco"]
        lres = []
        for k in range(self.n_lf):
            t, b = self.lf_arr[k], self.block_of_lf(k)
            n, po = b["w"] * b["h"], self.preds[t.pred][1]
            e = self.lf_job_expect(k, exp["pred"][po:po + n].reshape(b["h"], b["w"]), exp["resi"][po:po + n].reshape(b["h"], b["w"]))
            levels[t.outOff:t.outOff + n], reco[t.outOff:t.outOff + n] = e["levels"], e["reco"]
            lres.append(e["result"])
        exp.update(levels=levels, reco=reco, lf_results=lres)
        self._lexp = exp
        return exp

    def lf_oracle_expect(self, k):
        """without any device entry: the prediction from intra_util / mip_util"""
        import intra_util as iu
        import mip_util as mu
        t, b = self.lf_arr[k], self.block_of_lf(k)
        if t.pred < self.n_intra:
            pred = iu.predict(b["top"], b["left"], b["w"], b["h"], self.ij[t.pred][1], b["m"], b["bd"], [])
        else:
            _, mode, tr, _ = self.mj[t.pred - self.n_intra]
            pred = mu.predict(b["top"], b["left"], b["w"], b["h"], mode, tr, b["bd"])
        return self.lf_job_expect(k, pred, np.ascontiguousarray(self.org_of(b) - pred, np.int16))

    def check_lf(self, got, exp, levels=True):
        self.check(got, exp, levels)
        res = [tuple(int(v) for v in r) for r in got["lf_results"][:self.n_lf]]
        assert res == exp["lf_results"], [(k, a, b) for k, (a, b) in enumerate(zip(res, exp["lf_results"])) if a != b][:4]

    def lf_untouched(self, got):
        return self.untouched(got) and (got["lf_results"].view(np.uint8) == FILL).all()


def make_lfnst_level(rng, shapes, tus_of, lfnst_of, stride=97, lfnst_order=None):
    """as intra_chain_util.make_level; lfnst_of( p, block dict, is_mip ) -> the (qp, irap, lfnstIdx) candidates of prediction p"""
    base = icu.make_level(rng, shapes, tus_of, stride=stride)
    n_intra = base.n_intra
    lf = [(p, qp, irap, idx) for p, (i, _) in enumerate(base.preds) for qp, irap, idx in lfnst_of(p, base.blocks[i], p >= n_intra)]
    return LfnstLevel(base.blocks, base.plane, base.tus, lf, lfnst_order=lfnst_order)
