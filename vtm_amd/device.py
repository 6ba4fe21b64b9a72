"""Thin Python host layer over the C ABI: context, device buffers and the batched calls.

Plumbing only -- every computation happens in libvtmhip.so.  numpy arrays go in/out through
vtmhip_dev_alloc / vtmhip_h2d / vtmhip_d2h; torch users pass `tensor.data_ptr()` wherever a device pointer is
expected and `torch.cuda.current_stream().cuda_stream` to `Context.set_stream`."""
import ctypes as C

import numpy as np

from . import lib as _lib
from .lib import (AffineJob, DistJob, FracJob, FracResult, FullJob, IctJob, IfJob, IntraBlock, IntraChromaBlock, IntraChromaJob, IntraJob, IntraParams, IntraTuJob, IntraTuResult, CclmModel, JccrJob, JccrResult, LmcsJob, McJob, MeResult, MipJob, PelOpJob, PicParams, QuantJob,   # noqa: F401
                  SbtEstJob, SbtEstResult, SbtJob, SbtResult, ScaleJob, TrJob, TuJob, TuResult, TzJob, VtmHipError, WpDistJob, WpParam, WpPredJob, WtdJob)


class DevBuf:
    """A device allocation owned by a Context (freed with the context or explicitly)."""

    def __init__(self, ctx, nbytes, dtype=np.uint8, shape=None):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        self.dtype = np.dtype(dtype)
        self.shape = shape
        p = C.c_void_p()
        ctx._check(ctx.L.vtmhip_dev_alloc(ctx.h, self.nbytes, C.byref(p)))
        self.ptr = p.value
        ctx._bufs.append(self)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.ctx._keep.append(arr)   # the copy is asynchronous: keep the source alive until the next sync
        self.ctx._check(self.ctx.L.vtmhip_h2d(self.ctx.h, self.ptr, arr.ctypes.data, arr.nbytes))
        return self

    def to_host(self, dtype=None, shape=None):
        dtype = np.dtype(dtype or self.dtype)
        out = np.empty(self.nbytes // dtype.itemsize, dtype=dtype)
        self.ctx._check(self.ctx.L.vtmhip_d2h(self.ctx.h, out.ctypes.data, self.ptr, out.nbytes))
        self.ctx._keep.clear()
        shape = shape or self.shape
        return out.reshape(shape) if shape is not None else out

    def free(self):
        if self.ptr:
            self.ctx.L.vtmhip_dev_free(self.ctx.h, self.ptr)
            self.ptr = None


class Context:
    """One per process / GPU (reference analogue: one RdCost/InterSearch stack, EncLib.cpp:110-122)."""

    def __init__(self, device=0):
        self.L = _lib.load()
        h = C.c_void_p()
        st = self.L.vtmhip_create(device, C.byref(h))
        if st != _lib.OK:
            raise VtmHipError(st, self.L.vtmhip_status_string(st).decode())
        self.h = h
        self._bufs = []
        self._keep = []

    def _check(self, st):
        if st != _lib.OK:
            raise VtmHipError(st, self.L.vtmhip_last_error(self.h).decode())

    def close(self):
        if self.h:
            for b in self._bufs:
                b.free()
            self.L.vtmhip_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_stream(self, stream_ptr):
        self._check(self.L.vtmhip_set_stream(self.h, stream_ptr))

    def use_own_stream(self):
        self._check(self.L.vtmhip_use_own_stream(self.h))

    def sync(self):
        self._check(self.L.vtmhip_sync(self.h))
        self._keep.clear()

    def alloc(self, nbytes, dtype=np.uint8, shape=None):
        return DevBuf(self, nbytes, dtype, shape)

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        return DevBuf(self, max(arr.nbytes, 1), arr.dtype, arr.shape).upload(arr)

    def timer_start(self):
        self._check(self.L.vtmhip_timer_start(self.h))

    def timer_stop_ms(self):
        ms = C.c_float()
        self._check(self.L.vtmhip_timer_stop_ms(self.h, C.byref(ms)))
        return ms.value

    # ---- pointer-surface calls (host arrays) ------------------------------------------------------------------
    def xGetSAD(self, org, org_stride, cur, cur_stride, w, h, sub_shift=0, org_off=0, cur_off=0):
        d = C.c_uint64()
        self._check(self.L.vtmhip_xGetSAD(self.h, org.ctypes.data + 2 * org_off, org_stride, cur.ctypes.data + 2 * cur_off,
                                          cur_stride, w, h, sub_shift, C.byref(d)))
        return d.value

    def xGetHADs(self, org, org_stride, cur, cur_stride, w, h, org_off=0, cur_off=0):
        d = C.c_uint64()
        self._check(self.L.vtmhip_xGetHADs(self.h, org.ctypes.data + 2 * org_off, org_stride, cur.ctypes.data + 2 * cur_off,
                                           cur_stride, w, h, C.byref(d)))
        return d.value

    def xGetSSE(self, org, org_stride, cur, cur_stride, w, h, org_off=0, cur_off=0):
        d = C.c_uint64()
        self._check(self.L.vtmhip_xGetSSE(self.h, org.ctypes.data + 2 * org_off, org_stride, cur.ctypes.data + 2 * cur_off,
                                          cur_stride, w, h, C.byref(d)))
        return d.value

    def set_luma_level_weights(self, lut, luma_bd, signal_type, chroma_weight, inv_lut=None):
        """RdCost's luma-level weight table (float64, 1 << luma_bd entries), signal type and chroma weight, plus the reshaper's inverse LUT (int16) or None."""
        lut = np.ascontiguousarray(lut, np.float64)
        inv = None if inv_lut is None else np.ascontiguousarray(inv_lut, np.int16)
        assert lut.size >= 1 << luma_bd and (inv is None or inv.size >= 1 << luma_bd)
        self._check(self.L.vtmhip_set_luma_level_weights(self.h, lut.ctypes.data, luma_bd, signal_type, chroma_weight,
                                                         None if inv is None else inv.ctypes.data))

    def xGetSSE_WTD(self, org, org_stride, cur, cur_stride, w, h, comp_id, org_luma=None, org_luma_stride=0, cshift_x=0, cshift_y=0,
                    org_off=0, cur_off=0, luma_off=0):
        """DF_SSE*_WTD distFunc (raw, before the chroma m_distortionWeight) on host arrays; org_luma: the co-located luma original of a chroma block."""
        d = C.c_uint64()
        lp = None if org_luma is None else org_luma.ctypes.data + 2 * luma_off
        self._check(self.L.vtmhip_xGetSSE_WTD(self.h, org.ctypes.data + 2 * org_off, org_stride, cur.ctypes.data + 2 * cur_off, cur_stride, w, h,
                                              comp_id, lp, org_luma_stride, cshift_x, cshift_y, C.byref(d)))
        return d.value

    def sse_wtd_batch(self, d_org, d_cur, d_org_luma, d_jobs, n, d_out):
        """n WtdJob evaluations; d_out[i] = the raw distFunc value (WTD_INVALID_DIST for a rejected job)."""
        self._check(self.L.vtmhip_sse_wtd_batch_dev(self.h, d_org, d_cur, d_org_luma, d_jobs, n, d_out))

    def _wp_dist(self, fn, org, org_stride, cur, cur_stride, w, h, wp, bit_depth, is_bi, *max_dist):
        d = C.c_uint64()
        p = WpParam(*(int(v) for v in wp))
        self._check(fn(self.h, org.ctypes.data, org_stride, cur.ctypes.data, cur_stride, w, h, C.byref(p), bit_depth, int(is_bi), *max_dist, C.byref(d)))
        return d.value

    def xGetSADw(self, org, org_stride, cur, cur_stride, w, h, wp, bit_depth, is_bi, max_dist=(1 << 64) - 1):
        """RdCostWeightPrediction::xGetSADw on host arrays; wp = (w, offset, shift, round) of the component, max_dist the early-exit bound."""
        return self._wp_dist(self.L.vtmhip_xGetSADw, org, org_stride, cur, cur_stride, w, h, wp, bit_depth, is_bi, max_dist)

    def xGetSSEw(self, org, org_stride, cur, cur_stride, w, h, wp, bit_depth, is_bi):
        """RdCostWeightPrediction::xGetSSEw on host arrays."""
        return self._wp_dist(self.L.vtmhip_xGetSSEw, org, org_stride, cur, cur_stride, w, h, wp, bit_depth, is_bi)

    def xGetHADsw(self, org, org_stride, cur, cur_stride, w, h, wp, bit_depth, is_bi):
        """RdCostWeightPrediction::xGetHADsw (step 1) on host arrays."""
        return self._wp_dist(self.L.vtmhip_xGetHADsw, org, org_stride, cur, cur_stride, w, h, wp, bit_depth, is_bi)

    def wp_dist_batch(self, d_org, d_cur, d_jobs, n, d_out):
        """n WpDistJob evaluations; d_out[i] = the distFunc value (WP_INVALID_DIST for a rejected job)."""
        self._check(self.L.vtmhip_wp_dist_batch_dev(self.h, d_org, d_cur, d_jobs, n, d_out))

    def wp_pred_batch(self, d_src0, d_src1, d_dst, d_jobs, n):
        """n WpPredJob sample ops (addWeightUni / addWeightBi) on 14-bit intermediates."""
        self._check(self.L.vtmhip_wp_pred_batch_dev(self.h, d_src0, d_src1, d_dst, d_jobs, n))

    def xGetSADwMask(self, org, org_stride, cur, cur_stride, w, h, mask, mask_off, mask_stride, step_x, mask_stride2, sub_shift=0):
        """DF_SAD_WITH_MASK on host arrays; `mask` is a 1-D int16 array, mask_off the index of DistParam::mask inside it."""
        d = C.c_uint64()
        self._check(self.L.vtmhip_xGetSADwMask(self.h, org.ctypes.data, org_stride, cur.ctypes.data, cur_stride, w, h, sub_shift,
                                               mask.ctypes.data + 2 * mask_off, mask_stride, step_x, mask_stride2, C.byref(d)))
        return d.value

    def masked_sad_batch(self, d_org, d_cur, d_mask, d_jobs, n, d_dist):
        self._check(self.L.vtmhip_masked_sad_batch_dev(self.h, d_org, d_cur, d_mask, d_jobs, n, d_dist))

    def weightedGeoBlk(self, src0, src1, w, h, weight, weight_off, step_x, weight_stride, bit_depth=10, clip=None):
        """m_weightedGeoBlk on host arrays (h x w int16 blocks); `weight` is a 1-D int16 array, weight_off the index of the first weight."""
        clip = clip or (0, (1 << bit_depth) - 1)
        dst = np.zeros((h, w), np.int16)
        self._check(self.L.vtmhip_weightedGeoBlk(self.h, src0.ctypes.data, src0.strides[0] // 2, src1.ctypes.data, src1.strides[0] // 2, dst.ctypes.data, w,
                                                 w, h, weight.ctypes.data + 2 * weight_off, step_x, weight_stride, bit_depth, clip[0], clip[1]))
        return dst

    def weightedGeoBlk_batch(self, d_src, d_dst, d_weight, d_jobs, n, bit_depth=10, clip=None):
        clip = clip or (0, (1 << bit_depth) - 1)
        self._check(self.L.vtmhip_weightedGeoBlk_batch_dev(self.h, d_src, d_dst, d_weight, d_jobs, n, bit_depth, clip[0], clip[1]))

    def filter(self, vertical, taps, is_first, is_last, src, src_off, src_stride, w, h, coeff, bit_depth=10, clip=None, bimc=0):
        """m_filterHor/m_filterVer[taps][isFirst][isLast] on a host array; returns the h x w int16 block."""
        clip = clip or (0, (1 << bit_depth) - 1)
        dst = np.zeros((h, w), np.int16)
        co = np.ascontiguousarray(coeff, dtype=np.int16)
        fn = self.L.vtmhip_filterVer if vertical else self.L.vtmhip_filterHor
        self._check(fn(self.h, taps, is_first, is_last, src.ctypes.data + 2 * src_off, src_stride, dst.ctypes.data, w, w, h,
                       co.ctypes.data, bit_depth, clip[0], clip[1], bimc))
        return dst

    def filter_copy(self, is_first, is_last, src, src_off, src_stride, w, h, bit_depth=10, clip=None, bimc=0):
        clip = clip or (0, (1 << bit_depth) - 1)
        dst = np.zeros((h, w), np.int16)
        self._check(self.L.vtmhip_filterCopy(self.h, is_first, is_last, src.ctypes.data + 2 * src_off, src_stride, dst.ctypes.data,
                                             w, w, h, bit_depth, clip[0], clip[1], bimc))
        return dst

    def fastFwdTrans(self, ttype, n, src, shift, line, skip1, skip2):
        src = np.ascontiguousarray(src, dtype=np.int32)
        dst = np.zeros(n * line, np.int32)
        self._check(self.L.vtmhip_fastFwdTrans(self.h, ttype, n, src.ctypes.data, dst.ctypes.data, shift, line, skip1, skip2))
        return dst

    def fastInvTrans(self, ttype, n, src, shift, line, skip1, skip2, cmin=-32768, cmax=32767):
        src = np.ascontiguousarray(src, dtype=np.int32)
        dst = np.zeros(n * line, np.int32)
        self._check(self.L.vtmhip_fastInvTrans(self.h, ttype, n, src.ctypes.data, dst.ctypes.data, shift, line, skip1, skip2, cmin, cmax))
        return dst

    def fwdTransformCbCr(self, mode, cb, cr):
        """(*m_fwdICT[mode])(resCb, resCr, resC1, resC2) on two 2-D int16 host arrays (any row stride); returns (joint residual or None for mode 0, (d1, d2))."""
        h, w = cb.shape
        assert cr.shape == cb.shape and cb.strides[1] == 2 and cr.strides[1] == 2
        joint = np.zeros((h, w), np.int16) if mode else None
        jp = joint.ctypes.data if mode else None
        d = (C.c_int64 * 2)()
        self._check(self.L.vtmhip_fwdTransformCbCr(self.h, mode, cb.ctypes.data, cb.strides[0] // 2, cr.ctypes.data, cr.strides[0] // 2, jp, w, jp, w, w, h, d))
        return joint, (d[0], d[1])

    def invTransformCbCr(self, mode, cb, cr):
        """(*m_invICT[mode])(resCb, resCr), in place on two 2-D int16 host arrays (any row stride)."""
        h, w = cb.shape
        assert cr.shape == cb.shape and cb.strides[1] == 2 and cr.strides[1] == 2
        self._check(self.L.vtmhip_invTransformCbCr(self.h, mode, cb.ctypes.data, cb.strides[0] // 2, cr.ctypes.data, cr.strides[0] // 2, w, h))

    def set_lmcs_fwd_lut(self, fwd_lut, luma_bd):
        """The reshaper's forward LUT (int16, 1 << luma_bd entries) for lmcs_resi_batch / lmcs_reco_batch."""
        lut = np.ascontiguousarray(fwd_lut, np.int16)
        assert lut.size >= 1 << luma_bd
        self._check(self.L.vtmhip_set_lmcs_fwd_lut(self.h, lut.ctypes.data, luma_bd))

    def set_lmcs_inv_lut(self, inv_lut, luma_bd):
        """The reshaper's inverse LUT (int16, 1 << luma_bd entries) for ciip_cand_satd_batch; a slot of its own, beside set_luma_level_weights' inv_lut."""
        lut = np.ascontiguousarray(inv_lut, np.int16)
        assert lut.size >= 1 << luma_bd
        self._check(self.L.vtmhip_set_lmcs_inv_lut(self.h, lut.ctypes.data, luma_bd))

    def rspSignal(self, buf, lut):
        """AreaBuf<Pel>::rspSignal( lut ), in place on a 2-D int16 host array (any row stride)."""
        h, w = buf.shape
        lut = np.ascontiguousarray(lut, np.int16)
        assert buf.strides[1] == 2
        self._check(self.L.vtmhip_rspSignal(self.h, buf.ctypes.data, buf.strides[0] // 2, w, h, lut.ctypes.data, lut.size))

    def scaleSignal(self, buf, scale, fwd, bit_depth):
        """AreaBuf<Pel>::scaleSignal( scale, dir, clpRng ), in place on a 2-D int16 host array (any row stride)."""
        h, w = buf.shape
        assert buf.strides[1] == 2
        self._check(self.L.vtmhip_scaleSignal(self.h, buf.ctypes.data, buf.strides[0] // 2, w, h, scale, int(fwd), bit_depth))

    # ---- batched device calls (device pointers: DevBuf.ptr or tensor.data_ptr()) ---------------------------------
    def dist_batch(self, d_org, d_cur, d_jobs, n, d_out):
        self._check(self.L.vtmhip_dist_batch_dev(self.h, d_org, d_cur, d_jobs, n, d_out))

    def dist_uniform_batch(self, d_org, d_cur, d_jobs, n, kind, w, h, sub_shift, d_out):
        """Every job is w x h of one kind: small blocks share a wave (vtmhip_dist_uniform_batch_dev)."""
        self._check(self.L.vtmhip_dist_uniform_batch_dev(self.h, d_org, d_cur, d_jobs, n, kind, w, h, sub_shift, d_out))

    def satd8_grid(self, d_org, org_stride, d_ref, ref_stride, w, h, r, d_out):
        self._check(self.L.vtmhip_satd8_grid_dev(self.h, d_org, org_stride, d_ref, ref_stride, w, h, r, d_out))

    def if_batch(self, d_src, d_dst, d_jobs, n):
        self._check(self.L.vtmhip_if_batch_dev(self.h, d_src, d_dst, d_jobs, n))

    def frac_search_batch(self, d_org, d_ref, d_jobs, n, max_w, max_h, d_results, uniform_square=False):
        self._check(self.L.vtmhip_frac_search_batch_dev(self.h, d_org, d_ref, d_jobs, n, max_w, max_h, int(uniform_square), d_results))

    def xT_batch(self, d_resi, d_coef, d_jobs, n, max_w, max_h, d_sum_abs=None):
        self._check(self.L.vtmhip_xT_batch_dev(self.h, d_resi, d_coef, d_jobs, n, max_w, max_h, d_sum_abs))

    def xT_uniform_batch(self, d_resi, d_jobs, n, w, h, d_coef, d_results):
        """Forward transforms of n uniform w x h TUs (TuJob table): coefficients + sum|coef| (vtmhip_xT_uniform_batch_dev)."""
        self._check(self.L.vtmhip_xT_uniform_batch_dev(self.h, d_resi, d_jobs, n, w, h, d_coef, d_results))

    def xIT_batch(self, d_coef, d_resi, d_jobs, n, max_w, max_h):
        self._check(self.L.vtmhip_xIT_batch_dev(self.h, d_coef, d_resi, d_jobs, n, max_w, max_h))

    def quant_batch(self, d_coef, d_q, d_delta_u, d_jobs, n, d_abs_sum):
        self._check(self.L.vtmhip_quant_batch_dev(self.h, d_coef, d_q, d_delta_u, d_jobs, n, d_abs_sum))

    def dequant_batch(self, d_q, d_coef, d_jobs, n):
        self._check(self.L.vtmhip_dequant_batch_dev(self.h, d_q, d_coef, d_jobs, n))

    def full_search_batch(self, pic, d_org, d_ref, d_jobs, n, d_results, square=0, uniform=None):
        """square = S / uniform = (W, H): the caller promises S x S (W x H) jobs with searchRange <= 4 (lane-per-candidate kernel)."""
        if uniform:
            self._check(self.L.vtmhip_full_search_uniform_batch_dev(self.h, C.byref(pic), d_org, d_ref, d_jobs, n, uniform[0], uniform[1], d_results))
        elif square:
            self._check(self.L.vtmhip_full_search_square_batch_dev(self.h, C.byref(pic), d_org, d_ref, d_jobs, n, square, d_results))
        else:
            self._check(self.L.vtmhip_full_search_batch_dev(self.h, C.byref(pic), d_org, d_ref, d_jobs, n, d_results))

    def motion_estimation_batch(self, pic, cfg, d_org, d_ref, d_other, d_jobs, n, max_w, max_h, d_results):
        """InterSearch::xMotionEstimation for n (PU, list, refIdx) jobs (vtmhip_xMotionEstimation_batch_dev)."""
        self._check(self.L.vtmhip_xMotionEstimation_batch_dev(self.h, C.byref(pic), C.byref(cfg), d_org, d_ref, d_other, d_jobs, n,
                                                              max_w, max_h, d_results))

    def estimate_mvp_amvp_batch(self, pic, d_org, d_ref, d_jobs, n, max_w, max_h, uniform=False, add_idx_bits=True, d_dist_bip=None):
        """InterSearch::xEstimateMvPredAMVP (template cost of the AMVP candidates) for n MeJob rows, in place"""
        self._check(self.L.vtmhip_xEstimateMvPredAMVP_batch_dev(self.h, C.byref(pic), d_org, d_ref, d_jobs, n, max_w, max_h, int(uniform), int(add_idx_bits), d_dist_bip))

    def pis_run_picture(self, levels, n_levels, buffers, main_stream, side_streams):
        """the whole level-order chain of a picture in one native call (levels: ctypes array of PisLevelRun; side_streams: list of raw stream handles)"""
        arr = (C.c_void_p * max(1, len(side_streams)))(*side_streams)
        self._check(self.L.vtmhip_pis_run_picture(self.h, levels, n_levels, C.byref(buffers), C.c_void_p(main_stream), arr, len(side_streams)))

    def pred_inter_search_batch(self, level_run, buffers):
        """InterSearch::predInterSearch (translational part + SMVD block) of the n real PUs of `level_run` (a PisLevelRun with pis.candsGiven = 1) in one call"""
        self._check(self.L.vtmhip_predInterSearch_batch_dev(self.h, C.byref(level_run), C.byref(buffers)))

    def is_uniform_shape(self, w, h):
        return bool(self.L.vtmhip_is_uniform_shape(w, h))

    def tz_band_items(self, w, h, sub_shift, waves_per_job):
        """segments per thread of the row-band integer search kernel for a fused uniform launch of this shape; 0: the by-candidate kernel"""
        return int(self.L.vtmhip_tz_band_items(w, h, sub_shift, waves_per_job))

    def tz_box_sums(self, d_ref, d_sums, plane_off, stride, width, height, margin):
        """8x8 box sums of one luma plane (sample (0,0) at d_ref + plane_off) into the congruent uint16 buffer d_sums, for the raster pruning (vtmhip_tz_box_sums_dev)"""
        self._check(self.L.vtmhip_tz_box_sums_dev(self.h, d_ref, d_sums, plane_off, stride, width, height, margin))

    def tz_attach_sums(self, d_ref, d_sums, width=0, height=0, margin=0):
        """the TZ searches on d_ref use the box sums d_sums (computed with this width / height / margin) from now on; d_sums None: detach.  The caller keeps the sums
        current (vtmhip_tz_attach_sums)"""
        self._check(self.L.vtmhip_tz_attach_sums(self.h, d_ref if d_sums else None, d_sums, width, height, margin))

    def tz_prune_stats(self, reset=False):
        """raster pruning since the last reset: dict of scans listed / skipped / reduced / accepted and grid points evaluated / total (synchronises the stream)"""
        st = (C.c_uint64 * 6)()
        self._check(self.L.vtmhip_tz_prune_stats(self.h, st, int(reset)))
        return dict(zip(("listed", "skipped", "reduced", "points_evaluated", "points_total", "accepted"), (int(v) for v in st)))

    def tz_round_stats(self, reset=False):
        """round bound since the last reset: dict of rounds bounded / candidates listed / candidates skipped of the first and of the resume launches, and violations
        (evaluated candidates whose SAD was below their bound: 0) (synchronises the stream)"""
        st = (C.c_uint64 * 7)()
        self._check(self.L.vtmhip_tz_round_stats(self.h, st, int(reset)))
        return dict(zip(("first_rounds", "first_listed", "first_skipped", "resume_rounds", "resume_listed", "resume_skipped", "violations"), (int(v) for v in st)))

    def affine_motion_estimation_batch(self, pic, d_org, d_ref, d_other, d_jobs, n, max_w, max_h, d_results, bcw=False):
        """InterSearch::xAffineMotionEstimation per AffineMeJob (one workgroup per job); bcw: the batch may hold bi jobs under a CU-level BCW weight of -2 (32-bit variant beside)"""
        f = self.L.vtmhip_xAffineMotionEstimation_bcw_batch_dev if bcw else self.L.vtmhip_xAffineMotionEstimation_batch_dev
        self._check(f(self.h, C.byref(pic), d_org, d_ref, d_other, d_jobs, n, max_w, max_h, d_results))

    def mts_select_batch(self, d_results, num_tu, cands, w, h, bit_depth, max_cand, d_test):
        """TrQuant::transformNxN( trModes ) pre-selection of every TU of a level from the sum |coef| of its candidates (runs of num_tu results per candidate)"""
        arr = (C.c_uint8 * 8)(*cands)
        self._check(self.L.vtmhip_mts_select_batch_dev(self.h, d_results, num_tu, len(cands), arr, w, h, bit_depth, 15, max_cand, d_test))

    def smvd_batch(self, pic, d_org, d_ref, d_jobs, n, max_w, max_h, op, uniform=False):
        """the SMVD block of predInterSearch per SmvdJob, in place: op 0 xGetSymmetricCost, 1 xSymmetricMotionEstimation, 2 symmvdCheckBestMvp, 3 the whole block;
        uniform: every job is exactly max_w x max_h (VTMHIP_SMVD_UNIFORM: the lane-per-tile kernel for 8x8 .. 16x16)"""
        fn = (self.L.vtmhip_xGetSymmetricCost_batch_dev, self.L.vtmhip_xSymmetricMotionEstimation_batch_dev, self.L.vtmhip_symmvdCheckBestMvp_batch_dev)
        if op < 3 and not uniform:
            self._check(fn[op](self.h, C.byref(pic), d_org, d_ref, d_jobs, n, max_w, max_h))
        else:
            self._check(self.L.vtmhip_smvd_batch_dev(self.h, C.byref(pic), d_org, d_ref, d_jobs, n, max_w, max_h, op | (0x100 if uniform else 0)))

    def smvd_launch_form(self, max_w, max_h, bit_depth, uniform, n):
        """what smvd_batch launches for such a call: (kernel, waves per PU, candidate slots, PUs per wave) -- kernel 0 / 1 the general 64- / 256-lane kernel, 2 the
        tile kernel's group form, 3 its workgroup form (VTMHIP_SMVD_KERNEL_*)"""
        out = [C.c_int(-1) for _ in range(4)]
        self._check(self.L.vtmhip_smvd_launch_form(self.h, max_w, max_h, bit_depth, int(uniform), n, *[C.byref(v) for v in out]))
        return tuple(v.value for v in out)

    def pred_affine_blk_batch(self, pic, d_ref, d_dst, d_jobs, n, max_w, max_h):
        self._check(self.L.vtmhip_xPredAffineBlk_batch_dev(self.h, C.byref(pic), d_ref, d_dst, d_jobs, n, max_w, max_h))

    def lfnst_tu_batch(self, d_coef, d_jobs, n):
        """TrQuant::xFwdLfnst / xInvLfnst (gather, core multiply, scatter) in place on n TU coefficient blocks"""
        self._check(self.L.vtmhip_lfnst_tu_batch_dev(self.h, d_coef, d_jobs, n))

    def kernel_timing(self, enable):
        """HIP events around every launch of the main kernels, on the launch stream (vtmhip_kernel_timing)"""
        self._check(self.L.vtmhip_kernel_timing(self.h, int(enable)))

    def kernel_timing_read(self, kernel):
        """(total milliseconds, launches) of one kernel since kernel_timing(True)"""
        ms, n = C.c_double(), C.c_int()
        self._check(self.L.vtmhip_kernel_timing_read(self.h, kernel.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def merge_cand_satd_batch(self, pic, d_org, d_ref, d_pred, d_plain, n_plain, d_bdof, n_bdof, d_dmvr, n_dmvr, d_mvd, max_w, max_h, d_dist, uniform=False, use_satd=True):
        """merge-candidate SATD pre-selection (hook B10): predictions of the three candidate classes + Hadamard distortion"""
        self._check(self.L.vtmhip_merge_cand_satd_batch_dev(self.h, C.byref(pic), d_org, d_ref, d_pred, d_plain, n_plain, d_bdof, n_bdof, d_dmvr, n_dmvr, d_mvd, max_w, max_h,
                                                            int(uniform), int(use_satd), d_dist))

    def mmvd_cand_satd_batch(self, pic, d_org, d_ref, d_jobs, n, max_w, max_h, d_cand, d_dist, use_satd=True):
        """the MMVD loop of the same pre-selection: n MmvdJob CUs -> MmvdCand records and uint64 costs at [job * 64 + cand] (UINT64_MAX where kind == 0).  A malformed
        table is rejected whole (VtmHipError, nothing launched)."""
        self._check(self.L.vtmhip_mmvd_cand_satd_batch_dev(self.h, C.byref(pic), d_org, d_ref, d_jobs, n, max_w, max_h, int(use_satd), d_cand, d_dist))

    def ciip_cand_satd_batch(self, d_ref, d_line, d_org, d_pred, d_jobs, n, max_w, max_h, d_dist, use_satd=True, lmcs=False):
        """the CIIP loop of the same pre-selection: n CiipJob CUs -> uint64 costs at [job * 4 + cand] (UINT64_MAX from numCand on and in every slot of a malformed
        job, which the device skips); kept blocks at their keepOff inside d_pred.  Queues one launch: no read-back, no synchronisation.  lmcs: jobs may set
        their lmcs flag; both LUTs (set_lmcs_fwd_lut, set_lmcs_inv_lut) must then be there, of one depth."""
        self._check(self.L.vtmhip_ciip_cand_satd_batch_dev(self.h, d_ref, d_line, d_org, d_pred, d_jobs, n, max_w, max_h, int(use_satd), int(lmcs), d_dist))

    def ciip_blend_batch(self, d_line, d_pred, d_jobs, n):
        """geneWeightedPred in place for n CiipBlendJob blocks (luma and 4:2:0 chroma mixed); a malformed job is skipped on the device"""
        self._check(self.L.vtmhip_ciip_blend_batch_dev(self.h, d_line, d_pred, d_jobs, n))

    def geo_cand_satd_batch(self, d_ref, d_org, d_pred, d_jobs, n, max_w, max_h, d_result, d_sad_split=None, use_satd=True):
        """the GEO loop of the same pre-selection: n GeoJob CUs -> GeoResult records (whole SADs, the ordered list with SATD / SAD of each blend) and, where asked,
        the sadLarge table [job * 384 + split * 6 + cand]; kept 14-bit blocks go into d_pred.  Malformed jobs are skipped on the device; nothing is read back."""
        self._check(self.L.vtmhip_geo_cand_satd_batch_dev(self.h, d_ref, d_org, d_pred, d_jobs, n, max_w, max_h, int(use_satd), d_result, d_sad_split))

    def geo_blend_batch(self, d_src, d_dst, d_jobs, n):
        """weightedGeoBlk for n GeoCuBlendJob blocks (luma and 4:2:0 chroma), the weights from the closed form"""
        self._check(self.L.vtmhip_geo_blend_batch_dev(self.h, d_src, d_dst, d_jobs, n))

    def pis_stage(self, level, stage):
        self._check(self.L.vtmhip_pis_stage(self.h, C.byref(level), stage))

    def motion_compensation_batch(self, d_org, d_ref, d_pred, d_out, d_jobs, n, max_w, max_h):
        """InterPrediction::motionCompensation per PU (uni / bi + addAvg) with the fused residual / removeHighFreq epilogue."""
        self._check(self.L.vtmhip_motion_compensation_batch_dev(self.h, d_org, d_ref, d_pred, d_out, d_jobs, n, max_w, max_h))

    def bdof_batch(self, d_org, d_ref, d_pred, d_out, d_jobs, n, max_w, max_h):
        """xPredInterBi with bioApplied (BDOF) for bi-predicted luma PUs; same job table and epilogues as motion_compensation_batch."""
        self._check(self.L.vtmhip_bdof_batch_dev(self.h, d_org, d_ref, d_pred, d_out, d_jobs, n, max_w, max_h))

    def dmvr_batch(self, pic, d_org, d_ref, d_pred, d_out, d_jobs, n, max_w, max_h, d_mvd=0):
        """xProcessDMVR (luma) for bi-predicted merge PUs: refined prediction (+ epilogue) and the sub-PU vector differences."""
        self._check(self.L.vtmhip_dmvr_batch_dev(self.h, C.byref(pic), d_org, d_ref, d_pred, d_out, d_jobs, n, max_w, max_h, d_mvd))

    def dmvr_chroma_batch(self, pic, d_org, d_ref, d_pred, d_out, d_jobs, n, max_w, max_h, d_mvd):
        """One 4:2:0 chroma plane of the PUs of a dmvr_batch call (jobs address that plane; d_mvd from the luma call)."""
        self._check(self.L.vtmhip_dmvr_chroma_batch_dev(self.h, C.byref(pic), d_org, d_ref, d_pred, d_out, d_jobs, n, max_w, max_h, d_mvd))

    def lfnst_set_tables(self, lfnst8x8, lfnst4x4):
        """The caller's LFNST core matrices (int8 [4][2][16][48] and [4][2][16][16]), once per context."""
        a, b = np.ascontiguousarray(lfnst8x8, np.int8), np.ascontiguousarray(lfnst4x4, np.int8)
        assert a.size == 4 * 2 * 16 * 48 and b.size == 4 * 2 * 16 * 16
        self._check(self.L.vtmhip_lfnst_set_tables(self.h, a.ctypes.data, b.ctypes.data))

    def mip_set_tables(self, m4x4, m8x8, m16x16):
        """The caller's MIP matrices (uint8 mipMatrix4x4 [16][16][4], mipMatrix8x8 [8][16][8], mipMatrix16x16 [6][64][7]), once per context."""
        a, b, c = (np.ascontiguousarray(m, np.uint8) for m in (m4x4, m8x8, m16x16))
        assert a.size == 16 * 16 * 4 and b.size == 8 * 16 * 8 and c.size == 6 * 64 * 7
        self._check(self.L.vtmhip_mip_set_tables(self.h, a.ctypes.data, b.ctypes.data, c.ctypes.data))

    def lfnst(self, inverse, src, mode, index, size, zero_out):
        """TrQuant::fwdLfnstNxN / invLfnstNxN on a host vector; returns the trSize outputs."""
        src = np.ascontiguousarray(src, np.int32)
        dst = np.zeros(48 if size > 4 else 16, np.int32)
        fn = self.L.vtmhip_invLfnstNxN if inverse else self.L.vtmhip_fwdLfnstNxN
        self._check(fn(self.h, src.ctypes.data, dst.ctypes.data, mode, index, size, zero_out))
        return dst

    def lfnst_batch(self, d_src, d_dst, d_jobs, n):
        self._check(self.L.vtmhip_lfnst_batch_dev(self.h, d_src, d_dst, d_jobs, n))

    def mc_batch(self, d_ref, d_dst, d_jobs, n, max_w, max_h):
        """xPredInterBlk for luma and 4:2:0 chroma blocks (McJob.chroma)."""
        self._check(self.L.vtmhip_mc_batch_dev(self.h, d_ref, d_dst, d_jobs, n, max_w, max_h))

    def mc_luma_batch(self, d_ref, d_dst, d_jobs, n, max_w, max_h):
        self._check(self.L.vtmhip_mc_luma_batch_dev(self.h, d_ref, d_dst, d_jobs, n, max_w, max_h))

    def remove_high_freq_batch(self, d_org, d_pred, d_dst, d_jobs, n):
        self._check(self.L.vtmhip_remove_high_freq_batch_dev(self.h, d_org, d_pred, d_dst, d_jobs, n))

    def subtract_batch(self, d_a, d_b, d_dst, d_jobs, n):
        self._check(self.L.vtmhip_subtract_batch_dev(self.h, d_a, d_b, d_dst, d_jobs, n))

    def add_avg_batch(self, d_a, d_b, d_dst, d_jobs, n):
        self._check(self.L.vtmhip_add_avg_batch_dev(self.h, d_a, d_b, d_dst, d_jobs, n))

    def remove_weight_high_freq_batch(self, d_org, d_pred, d_dst, d_jobs, n):
        """BCW bi-pred ME target (PelOpJob.bcwWeight = weight of the searched list)."""
        self._check(self.L.vtmhip_remove_weight_high_freq_batch_dev(self.h, d_org, d_pred, d_dst, d_jobs, n))

    def add_weighted_avg_batch(self, d_a, d_b, d_dst, d_jobs, n):
        """BCW bi-prediction average (PelOpJob.bcwWeight = the list-1 weight)."""
        self._check(self.L.vtmhip_add_weighted_avg_batch_dev(self.h, d_a, d_b, d_dst, d_jobs, n))

    def tu_chain_batch(self, d_resi, d_jobs, n, max_w, max_h, d_results, d_levels=None, d_rec=None, uniform=False):
        self._check(self.L.vtmhip_tu_chain_batch_dev(self.h, d_resi, d_jobs, n, max_w, max_h, int(uniform), d_levels, d_rec, d_results))

    def tu_ts_chain_batch(self, d_resi, d_jobs, n, w, h, d_results, d_levels=None, d_rec=None):
        """transform-skip candidates (TuJob.typeHor == 3) of one TU size"""
        self._check(self.L.vtmhip_tu_ts_chain_batch_dev(self.h, d_resi, d_jobs, n, w, h, d_levels, d_rec, d_results))

    def ict_fwd_batch(self, d_resi, d_jobs, n, d_dist, d_joint=None):
        """forward ICT of cbfMask 0 .. 3 for n IctJob pairs: int64 d_dist[n][4][2] and the joint residual planes the jobs ask for"""
        self._check(self.L.vtmhip_ict_fwd_batch_dev(self.h, d_resi, d_jobs, n, d_joint, d_dist))

    def jccr_chain_batch(self, d_resi, d_jobs, n, max_w, max_h, d_results, d_levels=None, d_rec_cb=None, d_rec_cr=None, uniform=False):
        """the joint Cb-Cr candidate of n JccrJob pairs: forward ICT -> xT -> quant -> dequant -> xIT -> inverse ICT -> SSE of Cb and of Cr (JccrResult)"""
        self._check(self.L.vtmhip_jccr_chain_batch_dev(self.h, d_resi, d_jobs, n, max_w, max_h, int(uniform), d_levels, d_rec_cb, d_rec_cr, d_results))

    def tu_chain_crs_batch(self, d_resi, d_jobs, n, max_w, max_h, d_results, d_levels=None, d_rec=None, uniform=False):
        """tu_chain_batch with LMCS chroma residual scaling fused in: TuJob.chromaAdj = tu.getChromaAdj() or 0; sse against the unscaled residual"""
        self._check(self.L.vtmhip_tu_chain_crs_batch_dev(self.h, d_resi, d_jobs, n, max_w, max_h, int(uniform), d_levels, d_rec, d_results))

    def jccr_chain_crs_batch(self, d_resi, d_jobs, n, max_w, max_h, d_results, d_levels=None, d_rec_cb=None, d_rec_cr=None, uniform=False):
        """jccr_chain_batch with LMCS chroma residual scaling around the joint candidate: JccrJob.chromaAdj = tu.getChromaAdj() or 0"""
        self._check(self.L.vtmhip_jccr_chain_crs_batch_dev(self.h, d_resi, d_jobs, n, max_w, max_h, int(uniform), d_levels, d_rec_cb, d_rec_cr, d_results))

    def sbt_est_batch(self, d_org, d_pred, d_jobs, n, max_w, max_h, d_results):
        """InterSearch::calcMinDistSbt for n SbtEstJob CUs -> SbtEstResult (mode estimates, RDO order, skipAll, the raw partition sums)"""
        self._check(self.L.vtmhip_sbt_est_batch_dev(self.h, d_org, d_pred, d_jobs, n, max_w, max_h, d_results))

    def sbt_chain_batch(self, d_resi, d_jobs, n, d_results, d_levels=None, d_rec=None):
        """n SbtJob candidates (CU, sbtIdx, sbtPos): sub-TU expansion, the fused chain, completion over the whole CU -> SbtResult"""
        self._check(self.L.vtmhip_sbt_chain_batch_dev(self.h, d_resi, d_jobs, n, d_levels, d_rec, d_results))

    def intra_pred_batch(self, d_ref, d_blocks, num_blocks, d_jobs, n, d_pred):
        """predIntraAng (PDPC included) of n IntraJob (block, mode) pairs over num_blocks IntraBlock entries -> W x H samples, stride W, at IntraJob.predOff"""
        self._check(self.L.vtmhip_intra_pred_batch_dev(self.h, d_ref, d_blocks, num_blocks, d_jobs, n, d_pred))

    def intra_presel_batch(self, d_ref, d_org, d_blocks, num_blocks, d_jobs, n, d_dist):
        """the same predictions kept on chip: d_dist[2 k] = SAD, d_dist[2 k + 1] = SATD of job k against its block's original"""
        self._check(self.L.vtmhip_intra_presel_batch_dev(self.h, d_ref, d_org, d_blocks, num_blocks, d_jobs, n, d_dist))

    def intra_presel(self, blocks, org=None):
        """Host convenience over the two entries.  blocks: a list of dicts with `top`, `left` (numpy lines of 2W + 1 + m and 2H + 1 + m samples), `w`, `h`, `bd`,
        `m`, `modes` and -- for the pre-selection -- `org_off`, `org_stride` into the int16 plane `org`.  With `org` it returns a uint64 array [jobs, 2] of
        (SAD, SATD) in block-then-mode order, without it the list of predictions [h, w] in the same order."""
        tables, refs, acc = pack_intra_tables(blocks)
        blk_arr, job_arr, n = tables
        d_ref, d_blk, d_job = self.to_device(refs), self.to_device(struct_array_to_numpy(blk_arr)), self.to_device(struct_array_to_numpy(job_arr))
        if org is not None:
            d_org, d_out = self.to_device(np.ascontiguousarray(org, np.int16)), self.alloc(16 * n)
            self.intra_presel_batch(d_ref.ptr, d_org.ptr, d_blk.ptr, len(blocks), d_job.ptr, n, d_out.ptr)
            self.sync()
            res = d_out.to_host(np.uint64).reshape(n, 2)
        else:
            d_out = self.alloc(2 * max(acc, 1))
            self.intra_pred_batch(d_ref.ptr, d_blk.ptr, len(blocks), d_job.ptr, n, d_out.ptr)
            self.sync()
            flat = d_out.to_host(np.int16)
            res = [flat[j.predOff:j.predOff + blocks[j.block]["w"] * blocks[j.block]["h"]].reshape(blocks[j.block]["h"], blocks[j.block]["w"]) for j in job_arr]
        for b in (d_ref, d_blk, d_job, d_out) + ((d_org,) if org is not None else ()):
            b.free()
        return res

    def mip_pred_batch(self, d_ref, d_blocks, num_blocks, d_jobs, n, d_pred):
        """predBlock (MIP) of n MipJob (block, mode, transposed) triples over num_blocks IntraBlock entries -> W x H samples, stride W, at MipJob.predOff"""
        self._check(self.L.vtmhip_mip_pred_batch_dev(self.h, d_ref, d_blocks, num_blocks, d_jobs, n, d_pred))

    def mip_presel_batch(self, d_ref, d_org, d_blocks, num_blocks, d_jobs, n, d_dist):
        """the same predictions kept on chip: d_dist[2 k] = SAD, d_dist[2 k + 1] = SATD of job k against its block's original"""
        self._check(self.L.vtmhip_mip_presel_batch_dev(self.h, d_ref, d_org, d_blocks, num_blocks, d_jobs, n, d_dist))

    def intra_chain_batch(self, d_ref, d_org, d_blocks, num_blocks, d_intra_jobs, n_intra, d_mip_jobs, n_mip, d_tu_jobs, n_tu, d_pred, d_resi, d_reco, d_results,
                          d_levels=None):
        """one intra RD level: every prediction of the two job tables and its residual, then per IntraTuJob the fused chain, the clipped reconstruction (in place
        at outOff inside d_reco) and an IntraTuResult.  A malformed table is rejected whole (VtmHipError, nothing launched)."""
        self._check(self.L.vtmhip_intra_chain_batch_dev(self.h, d_ref, d_org, d_blocks, num_blocks, d_intra_jobs, n_intra, d_mip_jobs, n_mip, d_tu_jobs, n_tu,
                                                        d_pred, d_resi, d_levels, d_reco, d_results))

    def intra_chain_lfnst_batch(self, d_ref, d_org, d_blocks, num_blocks, d_intra_jobs, n_intra, d_mip_jobs, n_mip, d_tu_jobs, n_tu, d_lfnst_jobs, n_lfnst, d_pred, d_resi,
                                d_reco, d_results, d_lfnst_results, d_levels=None):
        """intra_chain_batch with a second candidate table: the IntraLfnstTuJob candidates (lfnstIdx 1 / 2) go through the LFNST chain on the same predictions and
        residuals, their IntraTuResult records to d_lfnst_results.  A malformed table is rejected whole (VtmHipError, nothing launched)."""
        self._check(self.L.vtmhip_intra_chain_lfnst_batch_dev(self.h, d_ref, d_org, d_blocks, num_blocks, d_intra_jobs, n_intra, d_mip_jobs, n_mip, d_tu_jobs, n_tu,
                                                              d_lfnst_jobs, n_lfnst, d_pred, d_resi, d_levels, d_reco, d_results, d_lfnst_results))

    def lfnst_chain_batch(self, d_resi, d_jobs, n, d_results, d_levels=None, d_rec=None):
        """the LFNST candidate of n LfnstChainJob TUs: kept-region xT -> forward LFNST -> quant of 8 / 16 positions -> dequant -> inverse LFNST -> xIT -> SSE (TuResult)"""
        self._check(self.L.vtmhip_lfnst_chain_batch_dev(self.h, d_resi, d_jobs, n, d_levels, d_rec, d_results))

    def isp_chain_batch(self, d_ref, d_org, d_blocks, num_blocks, d_jobs, n, d_reco, d_results, d_pred=None, d_levels=None):
        """n IspJob candidates (CU, mode, split) over num_blocks IntraBlock entries, every sub-partition of a candidate in one kernel: the W x H reconstruction at
        outOff inside d_reco, an IspResult per job, optionally the assembled prediction (predOff inside d_pred) and the levels (outOff inside d_levels, one TU-shaped
        block per sub-partition).  A malformed table is rejected whole (VtmHipError, nothing launched)."""
        self._check(self.L.vtmhip_isp_chain_batch_dev(self.h, d_ref, d_org, d_blocks, num_blocks, d_jobs, n, d_pred, d_levels, d_reco, d_results))

    def intra_chroma_pred_batch(self, d_ref, d_luma, d_blocks, num_blocks, d_jobs, n, d_pred):
        """the Cb and Cr predictions (regular modes 0 .. 66, LM 67, MDLM_L 68, MDLM_T 69) of n IntraChromaJob pairs over num_blocks IntraChromaBlock entries"""
        self._check(self.L.vtmhip_intra_chroma_pred_batch_dev(self.h, d_ref, d_luma, d_blocks, num_blocks, d_jobs, n, d_pred))

    def intra_chroma_presel_batch(self, d_ref, d_luma, d_org, d_blocks, num_blocks, d_jobs, n, d_dist):
        """the same predictions kept on chip: d_dist[4 k ..] = SAD Cb, SATD Cb, SAD Cr, SATD Cr of job k against its block's originals"""
        self._check(self.L.vtmhip_intra_chroma_presel_batch_dev(self.h, d_ref, d_luma, d_org, d_blocks, num_blocks, d_jobs, n, d_dist))

    def intra_chroma_presel(self, blocks, luma, org=None):
        """Host convenience over the two entries.  blocks: a list of dicts with `lines` = ((Cb top, Cb left), (Cr top, Cr left)) (numpy, 2W + 1 and 2H + 1 samples),
        `w`, `h`, `bd`, `above`, `left`, `ar`, `bl`, `first_row`, `coloc`, `luma_off`, `luma_stride` into the int16 array `luma`, `modes` and -- for the
        pre-selection -- `org_off` = (Cb, Cr), `org_stride` into the int16 array `org`.  With `org` it returns a uint64 array [jobs, 4] of (SAD Cb, SATD Cb, SAD Cr,
        SATD Cr) in block-then-mode order, without it the list of predictions [2, h, w] in the same order."""
        tables, refs, acc = pack_intra_chroma_tables(blocks)
        blk_arr, job_arr, n = tables
        bufs = [self.to_device(refs), self.to_device(np.ascontiguousarray(luma, np.int16).reshape(-1)), self.to_device(struct_array_to_numpy(blk_arr)),
                self.to_device(struct_array_to_numpy(job_arr))]
        d_ref, d_luma, d_blk, d_job = bufs
        if org is not None:
            bufs += [self.to_device(np.ascontiguousarray(org, np.int16).reshape(-1)), self.alloc(32 * max(n, 1))]
            self.intra_chroma_presel_batch(d_ref.ptr, d_luma.ptr, bufs[4].ptr, d_blk.ptr, len(blocks), d_job.ptr, n, bufs[5].ptr)
            self.sync()
            res = bufs[5].to_host(np.uint64).reshape(-1, 4)[:n]
        else:
            bufs.append(self.alloc(2 * max(acc, 1)))
            self.intra_chroma_pred_batch(d_ref.ptr, d_luma.ptr, d_blk.ptr, len(blocks), d_job.ptr, n, bufs[4].ptr)
            self.sync()
            flat = bufs[4].to_host(np.int16)
            res = [flat[j.cbPredOff:j.cbPredOff + 2 * blocks[j.block]["w"] * blocks[j.block]["h"]].reshape(2, blocks[j.block]["h"], blocks[j.block]["w"])
                   for j in job_arr[:n]]
        for b in bufs:
            b.free()
        return res

    def intra_chroma_chain_batch(self, d_ref, d_luma, d_org, d_blocks, num_blocks, d_jobs, n_pred, d_tu_jobs, n_tu, d_joint_jobs, n_joint, d_pred, d_resi, d_reco,
                                 d_reco_cr, d_results, d_joint_results, d_levels=None):
        """one intra chroma RD level: both predictions of every IntraChromaJob and their residuals, then per IntraChromaTuJob (one component) and per
        IntraChromaJointJob (joint Cb-Cr) the chain with chroma residual scaling, the clipped reconstruction (in place at outOff inside d_reco / d_reco_cr) and an
        IntraTuResult / IntraChromaJointResult.  A malformed table is rejected whole (VtmHipError, nothing launched)."""
        self._check(self.L.vtmhip_intra_chroma_chain_batch_dev(self.h, d_ref, d_luma, d_org, d_blocks, num_blocks, d_jobs, n_pred, d_tu_jobs, n_tu, d_joint_jobs, n_joint,
                                                               d_pred, d_resi, d_levels, d_reco, d_reco_cr, d_results, d_joint_results))

    def scale_signal_batch(self, d_src, d_dst, d_jobs, n):
        """scaleSignal of n ScaleJob blocks, each with its own scale and direction (d_dst may be d_src: in place)"""
        self._check(self.L.vtmhip_scale_signal_batch_dev(self.h, d_src, d_dst, d_jobs, n))

    def lmcs_resi_batch(self, d_org, d_pred, d_resi, d_jobs, n, d_dst=None):
        """resi = fwdLUT[org] - (MAP_PRED ? fwdLUT[pred] : pred) for n LmcsJob blocks; WRITE_MAPPED jobs also write that prediction to d_dst"""
        self._check(self.L.vtmhip_lmcs_resi_batch_dev(self.h, d_org, d_pred, d_resi, d_dst, d_jobs, n))

    def lmcs_reco_batch(self, d_pred, d_resi, d_dst, d_jobs, n):
        """reco = clip((MAP_PRED ? fwdLUT[pred] : pred) + resi) for n LmcsJob blocks"""
        self._check(self.L.vtmhip_lmcs_reco_batch_dev(self.h, d_pred, d_resi, d_dst, d_jobs, n))

    def affine_sobel_batch(self, d_pred, d_deriv, d_jobs, n):
        self._check(self.L.vtmhip_affine_sobel_batch_dev(self.h, d_pred, d_deriv, d_jobs, n))

    def affine_equal_coeff_batch(self, d_resi, d_deriv, d_jobs, n, d_eq):
        self._check(self.L.vtmhip_affine_equal_coeff_batch_dev(self.h, d_resi, d_deriv, d_jobs, n, d_eq))

    def tz_search_batch(self, pic, d_org, d_ref, d_jobs, n, d_results):
        self._check(self.L.vtmhip_tz_search_batch_dev(self.h, C.byref(pic), d_org, d_ref, d_jobs, n, d_results))


def struct_array_to_numpy(arr):
    """ctypes array of Structures -> uint8 numpy view (for upload)."""
    return np.frombuffer(arr, dtype=np.uint8)


def intra_pred_params(w, h, mode, m=0):
    """initPredIntraParams of a luma block as an IntraParams record (host arithmetic, no device)"""
    p = IntraParams()
    st = _lib.load().vtmhip_intra_pred_params(w, h, mode, m, C.byref(p))
    if st != _lib.OK:
        raise VtmHipError(st)
    return p


def mip_pred_host(w, h, bd, mode, transposed, top, left, m4x4, m8x8, m16x16):
    """MIP prediction [h, w] of one block on the host (no device): top / left indexed as the lines of an IntraBlock (top[1 .. w], left[1 .. h] are read)"""
    top, left = np.ascontiguousarray(top, np.int16), np.ascontiguousarray(left, np.int16)
    a, b, c = (np.ascontiguousarray(m, np.uint8) for m in (m4x4, m8x8, m16x16))
    if top.size < w + 1 or left.size < h + 1 or a.size != 16 * 16 * 4 or b.size != 8 * 16 * 8 or c.size != 6 * 64 * 7:
        raise VtmHipError(_lib.E_INVALID)
    pred = np.zeros((max(h, 1), max(w, 1)), np.int16)
    st = _lib.load().vtmhip_mip_pred_host(w, h, bd, mode, transposed, top.ctypes.data, left.ctypes.data, a.ctypes.data, b.ctypes.data, c.ctypes.data, pred.ctypes.data)
    if st != _lib.OK:
        raise VtmHipError(st)
    return pred


def pack_intra_tables(blocks):
    """IntraBlock / IntraJob tables of a list of block dicts (see Context.intra_presel): ((blocks, jobs, n), the concatenated int16 lines, prediction samples)"""
    blk_arr = (IntraBlock * max(len(blocks), 1))()
    refs, jobs, ref_off, pred_off = [], [], 0, 0
    for i, b in enumerate(blocks):
        top, left = np.asarray(b["top"], np.int16), np.asarray(b["left"], np.int16)
        assert top.size == 2 * b["w"] + 1 + b["m"] and left.size == 2 * b["h"] + 1 + b["m"]
        blk_arr[i] = IntraBlock(ref_off, b.get("org_off", 0), b.get("org_stride", 0), b["w"], b["h"], b["bd"], b["m"])
        refs += [top, left]
        ref_off += top.size + left.size
        for mode in b["modes"]:
            jobs.append(IntraJob(pred_off, i, mode))
            pred_off += b["w"] * b["h"]
    job_arr = (IntraJob * max(len(jobs), 1))(*jobs)
    return (blk_arr, job_arr, len(jobs)), (np.concatenate(refs) if refs else np.zeros(1, np.int16)), pred_off


def chroma_block_record(b, cb_ref_off, cr_ref_off):
    """the IntraChromaBlock of a block dict (see Context.intra_chroma_presel) whose lines start at the two offsets"""
    org = b.get("org_off", (0, 0))
    return IntraChromaBlock(cb_ref_off, cr_ref_off, org[0], org[1], b["luma_off"], b.get("org_stride", 0), b["luma_stride"], b["w"], b["h"], b["ar"], b["bl"], b["bd"],
                            int(b["above"]), int(b["left"]), int(b["first_row"]), int(b["coloc"]))


def pack_intra_chroma_tables(blocks):
    """IntraChromaBlock / IntraChromaJob tables of a list of block dicts: ((blocks, jobs, n), the concatenated int16 lines, prediction samples); the Cr prediction
    of a job follows its Cb prediction"""
    blk_arr = (IntraChromaBlock * max(len(blocks), 1))()
    refs, jobs, ref_off, pred_off = [], [], 0, 0
    for i, b in enumerate(blocks):
        offs = []
        for top, left in b["lines"]:
            top, left = np.asarray(top, np.int16), np.asarray(left, np.int16)
            assert top.size == 2 * b["w"] + 1 and left.size == 2 * b["h"] + 1
            offs.append(ref_off)
            refs += [top, left]
            ref_off += top.size + left.size
        blk_arr[i] = chroma_block_record(b, offs[0], offs[1])
        for mode in b["modes"]:
            jobs.append(IntraChromaJob(pred_off, pred_off + b["w"] * b["h"], i, mode))
            pred_off += 2 * b["w"] * b["h"]
    job_arr = (IntraChromaJob * max(len(jobs), 1))(*jobs)
    return (blk_arr, job_arr, len(jobs)), (np.concatenate(refs) if refs else np.zeros(1, np.int16)), pred_off


def cclm_params(block, ref, luma, component, mode):
    """xGetLMParameters of one (block dict, component 0 Cb / 1 Cr, mode 67 .. 69) as (a, b, shift): host arithmetic on numpy arrays, no device.  The block's lines
    are taken from the int16 array `ref` at `ref_off` = (Cb, Cr), its luma from the int16 array `luma`."""
    ref, luma = np.ascontiguousarray(ref, np.int16), np.ascontiguousarray(luma, np.int16)
    rec, out = chroma_block_record(block, block["ref_off"][0], block["ref_off"][1]), CclmModel()
    st = _lib.load().vtmhip_cclm_params(C.byref(rec), ref.ctypes.data, luma.ctypes.data, component, mode, C.byref(out))
    if st != _lib.OK:
        raise VtmHipError(st)
    return out.a, out.b, out.shift


def ict_select(dist, is_intra):
    """TrQuant::selectICTCandidates' decision from the four (d1, d2) pairs: the cbfMasks to test (host only, no device)."""
    d = (C.c_int64 * 8)(*[int(v) for pair in dist for v in pair])
    masks, num = (C.c_int * 2)(), C.c_int()
    st = _lib.load().vtmhip_ict_select(d, int(is_intra), masks, C.byref(num))
    if st != _lib.OK:
        raise VtmHipError(st)
    return [masks[i] for i in range(num.value)]


def sbt_skip_by_rdcost(est, dist_scale, sbt_idx, sbt_pos, best_cost, dist_sbt_off, cost_sbt_off, root_cbf_sbt_off):
    """InterSearch::skipSbtByRDCost over an est[9] record (host arithmetic, no device): 0 .. 3 or 255"""
    e = (C.c_uint64 * 9)(*[int(v) for v in est])
    st = _lib.load().vtmhip_sbt_skip_by_rdcost(e, dist_scale, sbt_idx, sbt_pos, best_cost, int(dist_sbt_off), cost_sbt_off, int(root_cbf_sbt_off))
    if st < 0:
        raise VtmHipError(st)
    return st


def sbt_make_tu_jobs(jobs):
    """The host form of the chain's expansion: (TuJob array, tuIdx int32 [n, 3]) of an SbtJob ctypes array"""
    n = len(jobs)
    out, idx, num = (TuJob * (3 * n))(), np.zeros((n, 3), np.int32), C.c_int()
    st = _lib.load().vtmhip_sbt_make_tu_jobs(C.addressof(jobs), n, C.addressof(out), C.byref(num), idx.ctypes.data)
    if st != _lib.OK:
        raise VtmHipError(st)
    return (TuJob * num.value).from_buffer_copy(bytes(out)[:num.value * C.sizeof(TuJob)]), idx


def intra_chain_make_tu_jobs(blocks, intra_jobs, mip_jobs, tu_jobs):
    """The host form of the intra chain's checks and expansion over ctypes arrays (None: an empty table): (TuJob array, maxWidth, maxHeight, uniform)"""
    n = [0 if a is None else len(a) for a in (blocks, intra_jobs, mip_jobs, tu_jobs)]
    ptr = [None if a is None else C.addressof(a) for a in (blocks, intra_jobs, mip_jobs, tu_jobs)]
    out, mw, mh, uni = (TuJob * max(n[3], 1))(), C.c_int(), C.c_int(), C.c_int()
    st = _lib.load().vtmhip_intra_chain_make_tu_jobs(ptr[0], n[0], ptr[1], n[1], ptr[2], n[2], ptr[3], n[3], C.addressof(out), C.byref(mw), C.byref(mh), C.byref(uni))
    if st != _lib.OK:
        raise VtmHipError(st)
    return (TuJob * n[3]).from_buffer_copy(bytes(out)[:n[3] * C.sizeof(TuJob)]), mw.value, mh.value, uni.value


def lfnst_mode(width, height, intra_mode, is_mip=False):
    """(set index, transpose flag) of a prediction on a width x height luma block (vtmhip_lfnst_mode_host)"""
    s, t = C.c_int(), C.c_int()
    st = _lib.load().vtmhip_lfnst_mode_host(width, height, intra_mode, int(is_mip), C.byref(s), C.byref(t))
    if st != _lib.OK:
        raise VtmHipError(st)
    return s.value, t.value


def intra_chain_lfnst_make_jobs(blocks, intra_jobs, mip_jobs, tu_jobs, lfnst_jobs):
    """The host form of the LFNST level entry's checks and expansions over ctypes arrays (None: an empty table):
    (TuJob array, LfnstChainJob array, maxWidth, maxHeight, uniform, lanes per LFNST job)"""
    tabs = (blocks, intra_jobs, mip_jobs, tu_jobs, lfnst_jobs)
    n = [0 if a is None else len(a) for a in tabs]
    ptr = [None if a is None else C.addressof(a) for a in tabs]
    out, lout = (TuJob * max(n[3], 1))(), (_lib.LfnstChainJob * max(n[4], 1))()
    mw, mh, uni, lanes = C.c_int(), C.c_int(), C.c_int(), C.c_int()
    st = _lib.load().vtmhip_intra_chain_lfnst_make_jobs(ptr[0], n[0], ptr[1], n[1], ptr[2], n[2], ptr[3], n[3], ptr[4], n[4], C.addressof(out), C.addressof(lout),
                                                        C.byref(mw), C.byref(mh), C.byref(uni), C.byref(lanes))
    if st != _lib.OK:
        raise VtmHipError(st)
    return ((TuJob * n[3]).from_buffer_copy(bytes(out)[:n[3] * C.sizeof(TuJob)]),
            (_lib.LfnstChainJob * n[4]).from_buffer_copy(bytes(lout)[:n[4] * C.sizeof(_lib.LfnstChainJob)]), mw.value, mh.value, uni.value, lanes.value)


def intra_chroma_chain_make_jobs(blocks, jobs, tu_jobs, joint_jobs):
    """The host form of the intra chroma chain's checks and expansion over ctypes arrays (None: an empty table):
    (TuJob array, JccrJob array, (maxWidth, maxHeight, uniform) of the single jobs, the same of the joint jobs, crs)"""
    n = [0 if a is None else len(a) for a in (blocks, jobs, tu_jobs, joint_jobs)]
    ptr = [None if a is None else C.addressof(a) for a in (blocks, jobs, tu_jobs, joint_jobs)]
    out_tu, out_joint = (TuJob * max(n[2], 1))(), (JccrJob * max(n[3], 1))()
    mw, mh, uni_tu, uni_joint, crs = (C.c_int * 2)(), (C.c_int * 2)(), C.c_int(), C.c_int(), C.c_int()
    st = _lib.load().vtmhip_intra_chroma_chain_make_jobs(ptr[0], n[0], ptr[1], n[1], ptr[2], n[2], ptr[3], n[3], C.addressof(out_tu), C.addressof(out_joint), mw, mh,
                                                         C.byref(uni_tu), C.byref(uni_joint), C.byref(crs))
    if st != _lib.OK:
        raise VtmHipError(st)
    return ((TuJob * n[2]).from_buffer_copy(bytes(out_tu)[:n[2] * C.sizeof(TuJob)]), (JccrJob * n[3]).from_buffer_copy(bytes(out_joint)[:n[3] * C.sizeof(JccrJob)]),
            (mw[0], mh[0], uni_tu.value), (mw[1], mh[1], uni_joint.value), crs.value)
