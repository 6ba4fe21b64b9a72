"""Joint Cb-Cr residual coding (JCCR / ICT) for the tests: the reference's rules restated in numpy, the real template instantiations through
ctypes, job packing for the device entries and the expectation of the joint chain composed from the restatement and the oracle's transform steps.

Reference: CommonLib/TrQuant.cpp fwdTransformCbCr / invTransformCbCr :86-157, selectICTCandidates :633-687; g_ictModes Rom.cpp:527."""
import ctypes as C
import os

import numpy as np

import oracle_lib as ol

MODES = (-3, -2, -1, 0, 1, 2, 3)
ICT_MODES = ((0, 3, 1, 2), (0, -3, -1, -2))   # g_ictModes[signFlag][cbfMask]
DCT2, TRSKIP = 0, 3


def mode_of(sign_flag, cbf_mask):
    return ICT_MODES[int(sign_flag)][cbf_mask]


def mask_of(mode):
    return {0: 0, 1: 2, 2: 3, 3: 1}[abs(mode)]


def _pel(v):
    return v.astype(np.int64).astype(np.int16)   # Pel( int ): wraps


def _cdiv(a, b):
    return np.sign(a) * (np.abs(a) // b)          # C++ `/`: toward zero


def fwd_ict(mode, cb, cr):
    """fwdTransformCbCr<mode>: (joint residual as int16 or None for mode 0, (d1, d2)); cb, cr: int16 arrays of one shape."""
    cb64, cr64 = cb.astype(np.int64), cr.astype(np.int64)
    if mode == 0:
        return None, (int((cb64 * cb64).sum()), int((cr64 * cr64).sum()))
    s, am = (-1 if mode < 0 else 1), abs(mode)
    if am == 1:
        c = _pel(_cdiv(4 * cb64 + s * 2 * cr64, 5)).astype(np.int64)
        d = (cb64 - c) ** 2 + (cr64 - ((s * c) >> 1)) ** 2
    elif am == 2:
        c = _pel(_cdiv(cb64 + s * cr64, 2)).astype(np.int64)
        d = (cb64 - c) ** 2 + (cr64 - s * c) ** 2
    else:
        c = _pel(_cdiv(4 * cr64 + s * 2 * cb64, 5)).astype(np.int64)
        d = (cb64 - ((s * c) >> 1)) ** 2 + (cr64 - c) ** 2
    return c.astype(np.int16), (int(d.sum()), 0)


def inv_ict(mode, cb, cr):
    """invTransformCbCr<mode>: the two blocks after the call (new int16 arrays)."""
    cb, cr = cb.copy(), cr.copy()
    s, am = (-1 if mode < 0 else 1), abs(mode)
    if am == 1:
        cr = _pel((s * cb.astype(np.int64)) >> 1)
    elif mode == 2:
        cr = cb.copy()
    elif mode == -2:
        cr = np.where(cb == -32768, 32767, -cb.astype(np.int64)).astype(np.int16)
    elif am == 3:
        cb = _pel((s * cr.astype(np.int64)) >> 1)
    return cb, cr


def select_ict(dist, is_intra):
    """selectICTCandidates' decision (:637-686) from the four (d1, d2) pairs: the cbfMasks to test, in the reference's order."""
    if not is_intra:
        return [3]
    min1, min2, m1, m2 = min(int(dist[0][0]), int(dist[0][1])), (1 << 63) - 1, 0, 0
    for m in (1, 2, 3):
        d = int(dist[m][0])
        if d < min1:
            m2, min2 = m1, min1
            m1, min1 = m, d
        elif d < min2:
            m2, min2 = m, d
    out = [m1] if m1 else []
    if m2 and (min2 < (9 * min1) // 8 or (not m1 and min2 < (3 * min1) // 2)):   # distances are >= 0: // is C++ /
        out.append(m2)
    return out


def golden_cases():
    """tests/golden/jccr.npz (recorded from the real reference by tests/golden/gen_jccr_golden.py): (mode, cb, cr, joint, (d1, d2), rewritten block) per case"""
    z = np.load(os.path.join(ol.ROOT, "tests", "golden", "jccr.npz"))
    z = {k: z[k] for k in z.files}
    for k in range(len(z["mode"])):
        m, w, h, o = int(z["mode"][k]), int(z["w"][k]), int(z["h"][k]), int(z["off"][k])
        blk = lambda a: np.ascontiguousarray(z[a][o:o + w * h].reshape(h, w))   # noqa: E731
        yield m, blk("cb"), blk("cr"), blk("joint"), tuple(int(v) for v in z["dist"][k]), blk("inv")


# ---- the real templates (weak symbols of oracle/_ref/libvtmref.so) -------------------------------------------------------------------------------
class _AreaBuf(C.Structure):   # AreaBuf<Pel> (24 bytes): width 0, height 4, buf 8, stride 16 (the layout tests/wp_util.py checks)
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("buf", C.c_void_p), ("stride", C.c_int32), ("_pad", C.c_int32)]


class _Pair(C.Structure):      # std::pair<int64_t, int64_t>: returned in two registers
    _fields_ = [("first", C.c_int64), ("second", C.c_int64)]


def _tag(mode):
    return "Li%d" % mode if mode >= 0 else "Lin%d" % -mode


class RefICT:
    def __init__(self, L):
        self.fwd, self.inv = {}, {}
        for m in MODES:
            f = getattr(L, "_Z16fwdTransformCbCrI%sEESt4pairIllERK7AreaBufIsES5_RS3_S6_" % _tag(m))
            f.restype, f.argtypes = _Pair, [C.POINTER(_AreaBuf)] * 4
            g = getattr(L, "_Z16invTransformCbCrI%sEEvR7AreaBufIsES2_" % _tag(m))
            g.restype, g.argtypes = None, [C.POINTER(_AreaBuf)] * 2
            self.fwd[m], self.inv[m] = f, g

    @staticmethod
    def _area(a):
        return _AreaBuf(a.shape[1], a.shape[0], a.ctypes.data, a.strides[0] // 2)

    def fwd_ict(self, mode, cb, cr):
        cb, cr = np.ascontiguousarray(cb, np.int16), np.ascontiguousarray(cr, np.int16)
        c1, c2 = np.full(cb.shape, 0x5555, np.int16), np.full(cb.shape, 0x5555, np.int16)
        a = [self._area(x) for x in (cb, cr, c1, c2)]
        p = self.fwd[mode](*[C.byref(x) for x in a])
        return (None if mode == 0 else (c2 if abs(mode) == 3 else c1)), (p.first, p.second)

    def inv_ict(self, mode, cb, cr):
        cb, cr = np.array(cb, np.int16, order="C"), np.array(cr, np.int16, order="C")
        a, b = self._area(cb), self._area(cr)
        self.inv[mode](C.byref(a), C.byref(b))
        return cb, cr


def random_pair(rng, w, h, amp, full_range=False):
    """(cb, cr) int16 blocks of amplitude amp; full_range: a few samples at the int16 limits (the Pel wrap, -32768 for mode -2)."""
    lo, hi = max(-amp, -32768), min(amp, 32767)
    cb, cr = rng.integers(lo, hi + 1, (h, w)).astype(np.int16), rng.integers(lo, hi + 1, (h, w)).astype(np.int16)
    if full_range:
        n = w * h
        for blk in (cb, cr):
            idx = rng.integers(0, n, max(1, n // 4))
            blk.reshape(-1)[idx] = rng.choice(np.array([-32768, -32767, 32767, 32766], np.int16), idx.size)
    return cb, cr


# ---- the joint chain ----------------------------------------------------------------------------------------------------------------------------
def chain_expect(cb, cr, cbf_mask, sign_flag, bd, qp_per, qp_rem, irap, ts):
    """The joint candidate of one (Cb, Cr) pair as the reference runs it: forward ICT, xT -> quant -> dequant -> xIT (or the transform-skip copies)
    on the joint residual through the oracle, inverse ICT, DF_SSE against the original residuals.  Returns a dict of everything the device reports."""
    L = ol.oracle()
    h, w = cb.shape
    mode = mode_of(sign_flag, cbf_mask)
    joint, (d1, _d2) = fwd_ict(mode, cb, cr)
    joint = np.ascontiguousarray(joint)
    coef, qc, dq = np.zeros(w * h, np.int32), np.zeros(w * h, np.int32), np.zeros(w * h, np.int32)
    s = C.c_int32()
    rec = np.zeros((h, w), np.int16)
    if ts:
        coef[:] = joint.reshape(-1)
        L.vo_quant(ol.P(coef), w, h, bd, qp_per, qp_rem, irap, 1, ol.P(qc), None, C.byref(s))
        L.vo_dequant(ol.P(qc), w, h, bd, qp_per, qp_rem, 1, ol.P(dq))
        rec[:] = dq.reshape(h, w).astype(np.int16)
    else:
        assert L.vo_fwd_2d(ol.P(joint), w, w, h, bd, 0, 0, ol.P(coef)) == 0
        L.vo_quant(ol.P(coef), w, h, bd, qp_per, qp_rem, irap, 0, ol.P(qc), None, C.byref(s))
        L.vo_dequant(ol.P(qc), w, h, bd, qp_per, qp_rem, 0, ol.P(dq))
        assert L.vo_inv_2d(ol.P(dq), w, h, bd, 0, 0, ol.P(rec), w) == 0
    # the coded component's block holds the reconstructed joint residual, the inverse ICT derives the other one
    if abs(mode) == 3:
        rec_cb, rec_cr = inv_ict(mode, np.zeros_like(rec), rec)
    else:
        rec_cb, rec_cr = inv_ict(mode, rec, np.zeros_like(rec))
    cb_c, cr_c = np.ascontiguousarray(cb), np.ascontiguousarray(cr)
    return dict(sseCb=ol.o_dist(2, cb_c, np.ascontiguousarray(rec_cb), w, h), sseCr=ol.o_dist(2, cr_c, np.ascontiguousarray(rec_cr), w, h), fwdDist=d1,
                sumAbs=int(np.abs(coef.astype(np.int64)).sum()), absSum=s.value, levels=qc, recCb=rec_cb.reshape(-1), recCr=rec_cr.reshape(-1), joint=joint)


def recipe_pair(rng, w, h, bd, amp, mode):
    """The input recipe of the chain tests: cb uniform in +-amp, cr = clip( s * cb * k // 4 + noise( +-amp / 4 ) ), k in 1 .. 4."""
    s, lim = (-1 if mode < 0 else 1), (1 << bd) - 1
    cb = rng.integers(-amp, amp + 1, (h, w)).astype(np.int64)
    k = int(rng.integers(1, 5))
    noise = rng.integers(-(amp // 4), amp // 4 + 1, (h, w))
    cr = np.clip(s * cb * k // 4 + noise, -lim, lim)
    return cb.astype(np.int16), cr.astype(np.int16)


class ChainBatch:
    """A batch of joint-chain jobs: the residual plane (Cb block and Cr block side by side per job), the JccrJob table and the expectations (computed
    once, in the constructor)."""

    def __init__(self, specs, bd, stride=144, out_slot=4096, cb_col=4):
        """specs: list of (cb, cr, cbf_mask, sign_flag, qp_per, qp_rem, irap, ts)"""
        from vtm_amd.lib import JccrJob
        n = len(specs)
        self.n, self.bd, self.slot = n, bd, out_slot
        self.resi = np.zeros((n * 64, stride), np.int16)
        self.jobs = (JccrJob * n)()
        self.exp = []
        for k, (cb, cr, mask, sign, per, rem, irap, ts) in enumerate(specs):
            h, w = cb.shape
            # Cb at column cb_col, Cr 68 columns on: with the default both offsets and the stride are multiples of 4 samples (the lane kernel's wide loads)
            self.resi[k * 64:k * 64 + h, cb_col:cb_col + w] = cb
            self.resi[k * 64:k * 64 + h, cb_col + 68:cb_col + 68 + w] = cr
            j = self.jobs[k]
            j.cbOff, j.crOff, j.outOff, j.resiStride = k * 64 * stride + cb_col, k * 64 * stride + cb_col + 68, k * out_slot, stride
            j.width, j.height, j.qpPer, j.qpRem, j.typeHor, j.bitDepth, j.isIRAP, j.cbfMask, j.signFlag = w, h, per, rem, TRSKIP if ts else DCT2, bd, irap, mask, sign
            self.exp.append(chain_expect(cb, cr, mask, sign, bd, per, rem, irap, ts))
        self.shapes = [(cb.shape[1], cb.shape[0]) for cb, *_ in specs]

    def run(self, ctx, max_w, max_h, uniform=False, idx=None):
        """Runs jobs idx (default: all) in one launch; returns (results, levels, recCb, recCr) as numpy / ctypes data for those jobs."""
        from vtm_amd.lib import JccrJob, JccrResult
        idx = list(range(self.n)) if idx is None else idx
        sub = (JccrJob * len(idx))()
        for i, k in enumerate(idx):
            C.memmove(C.byref(sub[i]), C.byref(self.jobs[k]), C.sizeof(JccrJob))
        d_resi, d_jobs = ctx.to_device(self.resi), ctx.to_device(np.frombuffer(sub, np.uint8))
        d_res = ctx.alloc(C.sizeof(JccrResult) * len(idx))
        d_lv = ctx.to_device(np.full((self.n, self.slot), -7, np.int32))
        d_cb, d_cr = ctx.to_device(np.full((self.n, self.slot), -7, np.int16)), ctx.to_device(np.full((self.n, self.slot), -7, np.int16))
        ctx.jccr_chain_batch(d_resi.ptr, d_jobs.ptr, len(idx), max_w, max_h, d_res.ptr, d_lv.ptr, d_cb.ptr, d_cr.ptr, uniform=uniform)
        res = (JccrResult * len(idx)).from_buffer_copy(d_res.to_host(np.uint8).tobytes())
        out = res, d_lv.to_host().reshape(self.n, self.slot), d_cb.to_host().reshape(self.n, self.slot), d_cr.to_host().reshape(self.n, self.slot)
        for d in (d_resi, d_jobs, d_res, d_lv, d_cb, d_cr):
            d.free()
        return out

    def check(self, got, idx=None):
        res, lv, rcb, rcr = got
        idx = list(range(self.n)) if idx is None else idx
        for i, k in enumerate(idx):
            e, (w, h), r = self.exp[k], self.shapes[k], res[i]
            tag = (k, w, h, self.bd, self.jobs[k].cbfMask, self.jobs[k].signFlag, self.jobs[k].typeHor, self.jobs[k].qpPer, self.jobs[k].qpRem)
            g = (r.sseCb, r.sseCr, r.fwdDist, r.sumAbs, r.absSum)
            assert g == (e["sseCb"], e["sseCr"], e["fwdDist"], e["sumAbs"], e["absSum"]), (tag, g, e)
            assert np.array_equal(lv[k, :w * h], e["levels"]), ("levels", tag)
            assert np.array_equal(rcb[k, :w * h], e["recCb"]) and np.array_equal(rcr[k, :w * h], e["recCr"]), ("rec", tag)

    def coded_share(self, idx=None):
        idx = list(range(self.n)) if idx is None else idx
        return sum(self.exp[k]["absSum"] > 0 for k in idx) / float(len(idx))
