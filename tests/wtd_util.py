"""Luma-level-weighted SSE (DF_SSE_WTD .. DF_SSE16N_WTD): an independent numpy restatement of the reference rule, job packing for
vtmhip_sse_wtd_batch_dev, and the ctypes handle on the real reference's RdCost::getWeightedMSE (oracle/_ref/libvtmref.so).

The rule (reference CommonLib/RdCost.cpp:3055-3086 getWeightedMSE, summed by xGetSSE*_WTD :3088-3463, orgLuma addressing :3110-3116):
    d      = org - cur
    lumaLv = Y: org;  chroma: orgLuma[(x << cShiftX) + (y << cShiftY) * stride]
    w      = Y: LUT[lumaLv];  chroma: signalType in (SDR, HLG) ? chromaWeight : LUT[lumaLv]
    mse    = int32( ((int64)(w * 65536.0) * d * d + 32768) >> 16 )    (Intermediate_Int is int: truncated)
    sum   += uint64(int64(mse))"""
import ctypes as C

import numpy as np

SDR, PQ, HLG = 0, 1, 2
CF_SCALE = {"420": (1, 1), "422": (1, 0), "444": (0, 0)}   # getComponentScaleX / Y of a chroma component


def fixed_weights(w):
    """(int64_t)(weight * (double)(1 << 16)), RdCost.cpp:3082: C truncation toward zero."""
    return np.trunc(np.asarray(w, np.float64) * 65536.0).astype(np.int64)


def sse_wtd(org, cur, comp, lut, signal, chroma_w, org_luma=None, csx=0, csy=0, inv=None):
    """org, cur: (h, w) sample blocks; org_luma: the luma original with its origin at the block's co-located top-left (chroma only);
    inv: inverse reshape LUT applied to cur first (Y only). Returns the raw distFunc value as a Python int (uint64 arithmetic)."""
    org = np.asarray(org, np.int64)
    cur = np.asarray(cur, np.int64)
    if inv is not None:
        cur = np.asarray(inv, np.int64)[cur]
    h, w = org.shape
    if comp == 0:
        lv = org
    else:
        lv = np.asarray(org_luma, np.int64)[(np.arange(h) << csy)[:, None], (np.arange(w) << csx)[None, :]]
    return int(mse_samples(comp, org, cur, lv, lut, signal, chroma_w).astype(np.int64).astype(np.uint64).sum(dtype=np.uint64))


def mse_samples(comp, org, cur, lv, lut, signal, chroma_w):
    """getWeightedMSE per sample (uiShift = 0), vectorised: int32 array."""
    org, cur, lv = (np.asarray(a, np.int64) for a in (org, cur, lv))
    if comp != 0 and signal in (SDR, HLG):
        fx = np.full(org.shape, int(fixed_weights(chroma_w)), np.int64)
    else:
        fx = fixed_weights(lut)[lv]
    d = org - cur
    return ((fx * (d * d) + 32768) >> 16).astype(np.int32)            # int64 -> int32 wraps like the C conversion


def pq_table(bd):
    """The PQ table RdCost::initLumaLevelToWeightTableReshape builds (RdCost.cpp:2982-2992), restated."""
    i = np.arange(1 << bd, dtype=np.float64)
    x = i * 2.0 ** (10 - bd) if bd < 10 else (np.floor(i / 2 ** (bd - 10)) if bd > 10 else i)
    y = np.clip(0.015 * x - 1.5 - 6, -3, 6)
    return 2.0 ** (y / 3.0)


def random_table(rng, bd, lo=0.3, hi=3.0):
    return rng.uniform(lo, hi, 1 << bd)


def random_inv_lut(rng, bd):
    """A monotone inverse-reshape-like LUT into [0, 2^bd)."""
    n = 1 << bd
    steps = rng.uniform(0.5, 1.5, n)
    v = np.cumsum(steps)
    return np.clip(np.round(v / v[-1] * (n - 1)), 0, n - 1).astype(np.int16)


def pack_jobs(jobs):
    """jobs: dicts with orgOff, curOff, orgLumaOff, orgStride, curStride, orgLumaStride, width, height, compID, cShiftX, cShiftY, flags -> uint8 array"""
    from vtm_amd.lib import WtdJob
    arr = (WtdJob * len(jobs))()
    for a, j in zip(arr, jobs):
        for k, v in j.items():
            setattr(a, k, int(v))
    return np.frombuffer(arr, np.uint8).copy()


# ---- the real reference (oracle/_ref/libvtmref.so, built with -fvisibility=default) -----------------------------------------------------
class RefWeightedMSE:
    """RdCost::getWeightedMSE( int compIdx, Pel org, Pel cur, uint32_t uiShift, Pel orgLuma ) with its static state driven through the exported statics."""

    def __init__(self, L):
        self.L = L
        self.fn = L._ZN6RdCost14getWeightedMSEEissjs
        self.fn.restype = C.c_uint64
        self.fn.argtypes = [C.c_int, C.c_int16, C.c_int16, C.c_uint32, C.c_int16]
        self.signal = C.c_uint32.in_dll(L, "_ZN6RdCost12m_signalTypeE")
        self.luma_bd = C.c_int.in_dll(L, "_ZN6RdCost8m_lumaBDE")
        self.chroma_w = C.c_double.in_dll(L, "_ZN6RdCost14m_chromaWeightE")
        self._vec = C.c_void_p.in_dll(L, "_ZN6RdCost30m_reshapeLumaLevelToWeightPLUTE")   # std::vector<double>: _M_start first
        self._init = L._ZN6RdCost33initLumaLevelToWeightTableReshapeEv
        self._init.restype = None
        self._init.argtypes = [C.c_void_p]
        self._this = C.create_string_buffer(1 << 16)   # the member function only touches statics
        self.luma_bd.value = 12                          # the vectors are sized on the first call: make them hold every bit depth
        self.signal.value = SDR
        self._init(self._this)

    def set_state(self, bd, signal, chroma_w, lut=None):
        """lut None: the table the reference builds itself for the signal type (initLumaLevelToWeightTableReshape)."""
        self.luma_bd.value = bd
        self.signal.value = signal
        self.chroma_w.value = chroma_w
        if lut is None:
            self._init(self._this)
        else:
            C.memmove(self._vec.value, np.ascontiguousarray(lut, np.float64).ctypes.data, 8 << bd)

    def table(self, bd):
        out = np.empty(1 << bd, np.float64)
        C.memmove(out.ctypes.data, self._vec.value, 8 << bd)
        return out

    def mse(self, comp, o, c, luma):
        return self.fn(comp, int(o), int(c), 0, int(luma))

    def block(self, org, cur, comp, org_luma=None, csx=0, csy=0):
        """xGetSSE_WTD's loop over the reference's per-sample function (uiSum += getWeightedMSE(...), uint64)."""
        h, w = org.shape
        s = 0
        for y in range(h):
            for x in range(w):
                lv = org[y, x] if comp == 0 else org_luma[y << csy, x << csx]
                s = (s + self.mse(comp, org[y, x], cur[y, x], lv)) & ((1 << 64) - 1)
        return s
