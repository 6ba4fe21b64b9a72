"""LMCS residual path for the tests: the reference's two scaling rules and rspSignal restated in numpy, the real members through ctypes, job packing
for the device entries and the expectation of the chains with chroma residual scaling, composed from the restatement, the oracle's transform steps
and jccr_util's ICT.

Reference: CommonLib/Buffer.cpp rspSignal :399-413, scaleSignal :415-464; EncoderLib/InterSearch.cpp:6628-6632, 6728-6733, 6838-6842, 6977-6998."""
import ctypes as C
import os

import numpy as np

import jccr_util as ju
import oracle_lib as ol

CSCALE_FP_PREC = 11
DCT2, TRSKIP = 0, 3
MAP_PRED, WRITE_MAPPED = 1, 2
SCALES = (1, 255, 256, 2047, 2048, 2049, 2731, 16384, 32767)
# the samples and scales of the exhaustive launches in tests/test_gpu_lmcs.py
EDGE_VALUES = sorted(set(list(range(0, 65)) + [v for k in range(1, 13) for v in ((1 << k) - 1, 1 << k, (1 << k) + 1)] + [32767, 32768]))
EDGE_SCALES = sorted(set([256, 257, 511, 512, 513, 16383, 16384, 1, 2, 3, 32767, 32766, 2731, 2047, 2048, 2049] +
                         [v for k in range(2, 15) for v in ((1 << k) - 1, 1 << k, (1 << k) + 1)] +
                         [5, 7, 11, 13, 17, 251, 263, 521, 1021, 1031, 2053, 4093, 4099, 8191, 8209, 16381, 16411, 32749]))


def scale_signal(blk, scale, fwd, bd):
    """AreaBuf<Pel>::scaleSignal( scale, dir, clpRng ): a new int16 array.  `/` truncates (the operands are non-negative), sgn(0) = +1."""
    v = np.asarray(blk).astype(np.int64)
    m = (1 << bd) - 1
    if fwd:
        sign = np.where(v >= 0, 1, -1)
        q = ((np.abs(v) << CSCALE_FP_PREC) + (scale >> 1)) // scale
        return np.clip(sign * q, -m, m).astype(np.int16)
    c = np.clip(v, -m - 1, m)
    sign = np.where(c >= 0, 1, -1)
    r = sign * ((np.abs(c) * scale + (1 << (CSCALE_FP_PREC - 1))) >> CSCALE_FP_PREC)
    return np.clip(r, -32768, 32767).astype(np.int16)


def saturated(blk, scale, bd):
    """the samples the forward rule clips"""
    v = np.abs(np.asarray(blk).astype(np.int64))
    return ((v << CSCALE_FP_PREC) + (scale >> 1)) // scale > (1 << bd) - 1


def rsp_signal(blk, lut):
    """AreaBuf<Pel>::rspSignal( lut )"""
    return np.asarray(lut, np.int16)[np.asarray(blk).astype(np.int64)]


def effective_adj(adj, w, h):
    """what the CRS chains apply: nothing for adj 0 (or out of range on the plain chain), nothing for blocks of at most 4 samples (InterSearch.cpp:6628)"""
    return adj if 1 <= adj <= 32767 and w * h > 4 else 0


def make_lut(seed, bd, bins=16):
    """A monotone piecewise-linear forward LUT of `bins` pieces over 1 << bd codewords and its inverse-free twin for the tests: int16 [1 << bd]."""
    rng = np.random.default_rng(seed)
    n = 1 << bd
    wts = rng.integers(1, 9, bins).astype(np.float64)
    wts[rng.integers(0, bins)] = 0.25                       # a nearly flat piece
    knots = np.concatenate([[0.0], np.cumsum(wts) / wts.sum()]) * (n - 1)
    x = np.arange(n) * (bins / float(n))
    i = np.minimum(x.astype(np.int64), bins - 1)
    lut = knots[i] + (knots[i + 1] - knots[i]) * (x - i)
    lut = np.floor(lut + 0.5).astype(np.int16)
    assert (np.diff(lut.astype(np.int32)) >= 0).all() and lut[0] >= 0 and lut[-1] <= n - 1
    return lut


def golden():
    z = np.load(os.path.join(ol.ROOT, "tests", "golden", "lmcs.npz"))
    return {k: z[k] for k in z.files}


def golden_scale_cases(z=None):
    """tests/golden/lmcs.npz (recorded from the real reference by tests/golden/gen_lmcs_golden.py): (w, h, bd, fwd, scale, input block, output block)"""
    z = z or golden()
    for k in range(len(z["sc_w"])):
        w, h, o = int(z["sc_w"][k]), int(z["sc_h"][k]), int(z["sc_off"][k])
        yield w, h, int(z["sc_bd"][k]), int(z["sc_dir"][k]), int(z["sc_scale"][k]), z["sc_in"][o:o + w * h].reshape(h, w), z["sc_out"][o:o + w * h].reshape(h, w)


def golden_case_inputs():
    """the inputs of the recorded cases: shapes x bit depths x directions x scales x amplitudes (3, M, 32767 with samples at the int16 limits)"""
    rng = np.random.default_rng(2024)
    for (w, h) in [(2, 2), (2, 8), (4, 4), (8, 4), (16, 16), (8, 2)]:
        for bd in (8, 10, 12):
            m = (1 << bd) - 1
            for fwd in (1, 0):
                for scale in SCALES:
                    for amp in (3, m, 32767):
                        blk = rng.integers(-amp, amp + 1, (h, w)).astype(np.int16)
                        if amp == 32767:
                            idx = rng.permutation(w * h)[:3]
                            blk.reshape(-1)[idx] = np.array([32767, -32767, -32768], np.int16)
                        yield w, h, bd, fwd, scale, blk


# ---- the real members (oracle/_ref/libvtmref.so) ---------------------------------------------------------------------------------------------------
class _AreaBuf(C.Structure):   # AreaBuf<Pel> (24 bytes): width 0, height 4, buf 8, stride 16
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("buf", C.c_void_p), ("stride", C.c_int32), ("_pad", C.c_int32)]


class _ClpRng(C.Structure):
    _fields_ = [("min", C.c_int32), ("max", C.c_int32), ("bd", C.c_int32), ("n", C.c_int32)]


class _Vector(C.Structure):    # std::vector<Pel> under libstdc++: begin, end, end of storage
    _fields_ = [("begin", C.c_void_p), ("end", C.c_void_p), ("cap", C.c_void_p)]


class RefLmcs:
    def __init__(self, L):
        self.scale = getattr(L, "_ZN7AreaBufIsE11scaleSignalEibRK6ClpRng")
        self.scale.restype, self.scale.argtypes = None, [C.POINTER(_AreaBuf), C.c_int, C.c_bool, C.POINTER(_ClpRng)]
        self.rsp = getattr(L, "_ZN7AreaBufIsE9rspSignalERSt6vectorIsSaIsEE")
        self.rsp.restype, self.rsp.argtypes = None, [C.POINTER(_AreaBuf), C.POINTER(_Vector)]
        self.reco = getattr(L, "_ZN7AreaBufIsE11reconstructERKS_IKsES4_RK6ClpRng")
        self.reco.restype, self.reco.argtypes = None, [C.POINTER(_AreaBuf)] * 3 + [C.POINTER(_ClpRng)]

    @staticmethod
    def _area(a):
        return _AreaBuf(a.shape[1], a.shape[0], a.ctypes.data, a.strides[0] // 2)

    def scale_signal(self, blk, scale, fwd, bd):
        out = np.array(blk, np.int16, order="C")
        a, c = self._area(out), _ClpRng(0, (1 << bd) - 1, bd, 0)
        self.scale(C.byref(a), scale, bool(fwd), C.byref(c))
        return out

    def rsp_signal(self, blk, lut):
        out, lut = np.array(blk, np.int16, order="C"), np.ascontiguousarray(lut, np.int16)
        a, v = self._area(out), _Vector(lut.ctypes.data, lut.ctypes.data + lut.nbytes, lut.ctypes.data + lut.nbytes)
        self.rsp(C.byref(a), C.byref(v))
        return out

    def reconstruct(self, pred, resi, bd):
        pred, resi = np.ascontiguousarray(pred, np.int16), np.ascontiguousarray(resi, np.int16)
        out = np.zeros(pred.shape, np.int16)
        a, p, r, c = self._area(out), self._area(pred), self._area(resi), _ClpRng(0, (1 << bd) - 1, bd, 0)
        self.reco(C.byref(a), C.byref(p), C.byref(r), C.byref(c))
        return out


# ---- the luma ops ---------------------------------------------------------------------------------------------------------------------------------
def resi_expect(org, pred, lut, map_pred):
    p = rsp_signal(pred, lut) if map_pred else np.asarray(pred, np.int16)
    return (rsp_signal(org, lut).astype(np.int64) - p).astype(np.int16), p


def reco_expect(pred, resi, lut, map_pred, bd):
    p = rsp_signal(pred, lut) if map_pred else np.asarray(pred, np.int16)
    return np.clip(p.astype(np.int64) + resi, 0, (1 << bd) - 1).astype(np.int16)


# ---- the chains with CRS ----------------------------------------------------------------------------------------------------------------------------
def tu_chain_expect(r, adj, bd, qp_per, qp_rem, irap, ts):
    """One chroma TU as the reference runs it with LMCS on: scaleSignal( adj, 1 ), xT -> quant -> dequant -> xIT (or the transform-skip copies) through
    the oracle, scaleSignal( adj, 0 ), DF_SSE against the unscaled residual.  DCT2 / DCT2 (chroma)."""
    L = ol.oracle()
    h, w = r.shape
    a = effective_adj(adj, w, h)
    rs = np.ascontiguousarray(scale_signal(r, a, 1, bd) if a else r.astype(np.int16))
    coef, qc, dq = np.zeros(w * h, np.int32), np.zeros(w * h, np.int32), np.zeros(w * h, np.int32)
    s = C.c_int32()
    pre = np.zeros((h, w), np.int16)
    if ts:
        coef[:] = rs.reshape(-1)
        L.vo_quant(ol.P(coef), w, h, bd, qp_per, qp_rem, irap, 1, ol.P(qc), None, C.byref(s))
        L.vo_dequant(ol.P(qc), w, h, bd, qp_per, qp_rem, 1, ol.P(dq))
        pre[:] = dq.reshape(h, w).astype(np.int16)
    else:
        assert L.vo_fwd_2d(ol.P(rs), w, w, h, bd, 0, 0, ol.P(coef)) == 0
        L.vo_quant(ol.P(coef), w, h, bd, qp_per, qp_rem, irap, 0, ol.P(qc), None, C.byref(s))
        L.vo_dequant(ol.P(qc), w, h, bd, qp_per, qp_rem, 0, ol.P(dq))
        assert L.vo_inv_2d(ol.P(dq), w, h, bd, 0, 0, ol.P(pre), w) == 0
    rec = scale_signal(pre, a, 0, bd) if a else pre
    d = r.astype(np.int64) - rec
    return dict(sse=int((d * d).sum()), sumAbs=int(np.abs(coef.astype(np.int64)).sum()), absSum=s.value, levels=qc, rec=rec.reshape(-1), pre=pre, adj=a,
                sat=int(saturated(r, a, bd).sum()) if a else 0)


def jccr_chain_expect(cb, cr, adj, cbf_mask, sign_flag, bd, qp_per, qp_rem, irap, ts):
    """The joint candidate with LMCS on: scale Cb and Cr, jccr_util's chain on the scaled pair (its fwdDist is the distance on the scaled pair), inverse
    scaling of both rebuilt blocks, DF_SSE against the unscaled residuals."""
    h, w = cb.shape
    a = effective_adj(adj, w, h)
    scb, scr = (scale_signal(cb, a, 1, bd), scale_signal(cr, a, 1, bd)) if a else (cb, cr)
    e = ju.chain_expect(np.ascontiguousarray(scb), np.ascontiguousarray(scr), cbf_mask, sign_flag, bd, qp_per, qp_rem, irap, ts)
    pre_cb, pre_cr = e["recCb"].reshape(h, w), e["recCr"].reshape(h, w)
    rcb, rcr = (scale_signal(pre_cb, a, 0, bd), scale_signal(pre_cr, a, 0, bd)) if a else (pre_cb, pre_cr)
    db, dr = cb.astype(np.int64) - rcb, cr.astype(np.int64) - rcr
    m = (1 << bd) - 1
    return dict(sseCb=int((db * db).sum()), sseCr=int((dr * dr).sum()), fwdDist=e["fwdDist"], sumAbs=e["sumAbs"], absSum=e["absSum"], levels=e["levels"],
                recCb=rcb.reshape(-1), recCr=rcr.reshape(-1), adj=a, sat=int(saturated(cb, a, bd).sum() + saturated(cr, a, bd).sum()) if a else 0,
                pre_out=bool(((pre_cb < -m - 1) | (pre_cb > m) | (pre_cr < -m - 1) | (pre_cr > m)).any()))


class TuBatch:
    """A batch of plain-chain jobs with a chroma adjustment each: the residual plane, the TuJob table and the expectations (computed once)."""

    def __init__(self, specs, bd, stride=144, out_slot=4096, col=4):
        """specs: list of (r, adj, qp_per, qp_rem, irap, ts)"""
        from vtm_amd.lib import TuJob
        n = len(specs)
        self.n, self.bd, self.slot = n, bd, out_slot
        self.resi = np.zeros((n * 64, stride), np.int16)
        self.jobs = (TuJob * n)()
        self.exp, self.shapes, self.samples = [], [], []
        for k, (r, adj, per, rem, irap, ts) in enumerate(specs):
            h, w = r.shape
            self.resi[k * 64:k * 64 + h, col:col + w] = r
            j = self.jobs[k]
            j.resiOff, j.outOff, j.resiStride, j.width, j.height = k * 64 * stride + col, k * out_slot, stride, w, h
            j.qpPer, j.qpRem, j.typeHor, j.typeVer, j.bitDepth, j.isIRAP, j.chromaAdj = per, rem, TRSKIP if ts else DCT2, TRSKIP if ts else DCT2, bd, irap, adj
            self.exp.append(tu_chain_expect(r, adj, bd, per, rem, irap, ts))
            self.shapes.append((w, h))
            self.samples.append(w * h)

    def run(self, ctx, max_w, max_h, uniform=False, idx=None, crs=True, adj_override=None):
        """Runs jobs idx (default: all, in this order) in one launch of the CRS entry (crs=False: the plain entry); returns (results, levels, rec)."""
        from vtm_amd.lib import TuJob, TuResult
        idx = list(range(self.n)) if idx is None else idx
        sub = (TuJob * len(idx))()
        for i, k in enumerate(idx):
            C.memmove(C.byref(sub[i]), C.byref(self.jobs[k]), C.sizeof(TuJob))
            if adj_override is not None:
                sub[i].chromaAdj = adj_override
        d_resi, d_jobs = ctx.to_device(self.resi), ctx.to_device(np.frombuffer(sub, np.uint8))
        d_res = ctx.to_device(np.full(C.sizeof(TuResult) * len(idx), 0xA5, np.uint8))
        d_lv, d_rec = ctx.to_device(np.full((self.n, self.slot), -7, np.int32)), ctx.to_device(np.full((self.n, self.slot), -7, np.int16))
        fn = ctx.tu_chain_crs_batch if crs else ctx.tu_chain_batch
        fn(d_resi.ptr, d_jobs.ptr, len(idx), max_w, max_h, d_res.ptr, d_lv.ptr, d_rec.ptr, uniform=uniform)
        res = (TuResult * len(idx)).from_buffer_copy(d_res.to_host(np.uint8).tobytes())
        out = res, d_lv.to_host().reshape(self.n, self.slot), d_rec.to_host().reshape(self.n, self.slot)
        for d in (d_resi, d_jobs, d_res, d_lv, d_rec):
            d.free()
        return out

    def check(self, got, idx=None):
        res, lv, rec = got
        idx = list(range(self.n)) if idx is None else idx
        for i, k in enumerate(idx):
            e, (w, h), r, j = self.exp[k], self.shapes[k], res[i], self.jobs[k]
            tag = (k, w, h, self.bd, j.chromaAdj, j.typeHor, j.qpPer, j.qpRem)
            g = (r.sse, r.sumAbs, r.absSum)
            assert g == (e["sse"], e["sumAbs"], e["absSum"]), (tag, g, (e["sse"], e["sumAbs"], e["absSum"]))
            assert np.array_equal(lv[k, :w * h], e["levels"]), ("levels", tag)
            assert np.array_equal(rec[k, :w * h], e["rec"]), ("rec", tag)

    def assert_bites(self):
        """The conditions on the inputs (on the EXPECTED values, never on the device's): enough coded jobs, saturation in fwd() and the inverse's input clip."""
        assert sum(e["absSum"] > 0 for e in self.exp) * 2 >= self.n, "fewer than half the jobs are coded"
        small = [k for k in range(self.n) if 0 < self.exp[k]["adj"] <= 512]
        assert small and sum(self.exp[k]["sat"] for k in small) * 10 >= sum(self.samples[k] for k in small), "fwd() hardly saturates"
        m = (1 << self.bd) - 1
        assert any(e["adj"] and ((e["pre"] < -m - 1) | (e["pre"] > m)).any() for e in self.exp), "the inverse's input clip never acts"


class JccrBatch(ju.ChainBatch):
    """jccr_util.ChainBatch with a chroma adjustment per job and the CRS expectation."""

    def __init__(self, specs, bd, stride=144, out_slot=4096, cb_col=4):
        """specs: list of (cb, cr, adj, cbf_mask, sign_flag, qp_per, qp_rem, irap, ts); the plane layout is the base class's (it is not initialised: its
        expectation is the unscaled one)"""
        from vtm_amd.lib import JccrJob
        n = len(specs)
        self.n, self.bd, self.slot = n, bd, out_slot
        self.resi = np.zeros((n * 64, stride), np.int16)
        self.jobs = (JccrJob * n)()
        self.exp, self.shapes, self.samples = [], [], []
        for k, (cb, cr, adj, mask, sign, per, rem, irap, ts) in enumerate(specs):
            h, w = cb.shape
            self.resi[k * 64:k * 64 + h, cb_col:cb_col + w] = cb
            self.resi[k * 64:k * 64 + h, cb_col + 68:cb_col + 68 + w] = cr
            j = self.jobs[k]
            j.cbOff, j.crOff, j.outOff, j.resiStride = k * 64 * stride + cb_col, k * 64 * stride + cb_col + 68, k * out_slot, stride
            j.width, j.height, j.qpPer, j.qpRem, j.typeHor, j.bitDepth, j.isIRAP, j.cbfMask, j.signFlag = w, h, per, rem, TRSKIP if ts else DCT2, bd, irap, mask, sign
            j.chromaAdj = adj
            self.exp.append(jccr_chain_expect(cb, cr, adj, mask, sign, bd, per, rem, irap, ts))
            self.shapes.append((w, h))
            self.samples.append(2 * w * h)

    def run(self, ctx, max_w, max_h, uniform=False, idx=None, crs=True, adj_override=None):
        from vtm_amd.lib import JccrJob, JccrResult
        idx = list(range(self.n)) if idx is None else idx
        sub = (JccrJob * len(idx))()
        for i, k in enumerate(idx):
            C.memmove(C.byref(sub[i]), C.byref(self.jobs[k]), C.sizeof(JccrJob))
            if adj_override is not None:
                sub[i].chromaAdj = adj_override
        d_resi, d_jobs = ctx.to_device(self.resi), ctx.to_device(np.frombuffer(sub, np.uint8))
        d_res = ctx.to_device(np.full(C.sizeof(JccrResult) * len(idx), 0xA5, np.uint8))
        d_lv = ctx.to_device(np.full((self.n, self.slot), -7, np.int32))
        d_cb, d_cr = ctx.to_device(np.full((self.n, self.slot), -7, np.int16)), ctx.to_device(np.full((self.n, self.slot), -7, np.int16))
        fn = ctx.jccr_chain_crs_batch if crs else ctx.jccr_chain_batch
        fn(d_resi.ptr, d_jobs.ptr, len(idx), max_w, max_h, d_res.ptr, d_lv.ptr, d_cb.ptr, d_cr.ptr, uniform=uniform)
        res = (JccrResult * len(idx)).from_buffer_copy(d_res.to_host(np.uint8).tobytes())
        out = res, d_lv.to_host().reshape(self.n, self.slot), d_cb.to_host().reshape(self.n, self.slot), d_cr.to_host().reshape(self.n, self.slot)
        for d in (d_resi, d_jobs, d_res, d_lv, d_cb, d_cr):
            d.free()
        return out

    def assert_bites(self):
        assert sum(e["absSum"] > 0 for e in self.exp) * 2 >= self.n, "fewer than half the jobs are coded"
        small = [k for k in range(self.n) if 0 < self.exp[k]["adj"] <= 512]
        assert small and sum(self.exp[k]["sat"] for k in small) * 10 >= sum(self.samples[k] for k in small), "fwd() hardly saturates"
        assert any(e["adj"] and e["pre_out"] for e in self.exp), "the inverse's input clip never acts"


def raw_results(res, fields):
    return [tuple(getattr(r, f) for f in fields) for r in res]
