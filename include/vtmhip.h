/*
 * vtmhip.h -- C ABI of libvtmhip.so: MI355X (gfx950) implementation of the VTM 9.3 inter motion-estimation +
 * transform/quantisation hot path.  Plain pointers and sizes only; no C++ or torch types cross this boundary.
 *
 * Two layers:
 *   (1) POINTER-SURFACE calls (host pointers in, host results out): one entry point per slot of the reference's
 *       function-pointer dispatch surface, same argument meaning, so a `initRdCostHIP()`-style installer can
 *       trampoline into them.  They stage the operands to the device, run the SAME kernels as
 *       layer 2 with a batch of one and copy the result back: correct drop-ins, not fast ones (a launch costs more
 *       than the whole CPU call, SURVEY.md section 7 hard part 1).
 *   (2) BATCHED DEVICE calls (`*_dev`): operands already resident in HBM (device pointers), many jobs per launch,
 *       asynchronous on the context's stream.  This is the product path; the hooks B1..B10 of SURVEY.md Appendix B
 *       feed it.
 *
 * Reference interfaces replaced (paths relative to /root/reference/source/Lib):
 *   DistParam::distFunc / RdCost::m_afpDistortFunc[DF_SAD*|DF_HAD*|DF_SSE*]   CommonLib/RdCost.h:60,67-105,113; RdCost.cpp:125-217
 *   RdCost::getCostOfVectorWithPredictor                                       CommonLib/RdCost.h:301-315
 *   InterSearch::xTZSearch / xPatternSearch / xPatternSearchFracDIF            EncoderLib/InterSearch.cpp:3640-3976, 3566-3608, 4284-4339
 *   InterpolationFilter::m_filterHor/m_filterVer/m_filterCopy                  CommonLib/InterpolationFilter.h:93-96
 *   fastFwdTrans / fastInvTrans, TrQuant::xT / xIT                             CommonLib/TrQuant.cpp:69-81, 776-923
 *   Quant::quant / Quant::dequant (flat scaling list)                          CommonLib/Quant.cpp:955-1038, 357-482
 *   AffineGradientSearch::m_HorizontalSobelFilter/m_VerticalSobelFilter/m_EqualCoeffComputer  CommonLib/AffineGradientSearch.h:50-54
 *   PelBufferOps::removeHighFreq / addAvg                                      CommonLib/Buffer.h:64-81
 *
 * Types: Pel = int16_t, TCoeff = int32_t, Distortion = uint64_t (CommonLib/TypeDef.h:259-270).
 * Every function returns VTMHIP_OK (0) or a negative VTMHIP_E_* code and never throws; a C++ trampoline turns a
 * non-zero status into the reference's THROW (TypeDef.h:1065-1081).
 *
 * Threading: a context is NOT re-entrant.  It owns one staging area (pointer surface), one workspace and one "current stream"; use one
 * context per host thread (per encoder stack, as the reference keeps one RdCost / InterSearch / TrQuant per thread) and, in a multi-GPU
 * process, one per device.  Every entry point makes the context's device the calling thread's current HIP device.
 */
#ifndef VTMHIP_H
#define VTMHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VTMHIP_ABI_VERSION 6

enum
{
  VTMHIP_OK            = 0,
  VTMHIP_E_INVALID     = -1,   /* bad argument (the reference would THROW "Unsupported size" / CHECK) */
  VTMHIP_E_NODEVICE    = -2,   /* no HIP device / device index out of range */
  VTMHIP_E_HIP         = -3,   /* a HIP runtime call failed; see vtmhip_last_error() */
  VTMHIP_E_NOMEM       = -4,
  VTMHIP_E_UNSUPPORTED = -5    /* caller must keep its CPU path (useMR, step != 1, explicit scaling lists, ...; applyWeight: the vtmhip_xGet*w entries) */
};

enum { VTMHIP_DIST_SAD = 0, VTMHIP_DIST_SATD = 1, VTMHIP_DIST_SSE = 2 };
enum { VTMHIP_DCT2 = 0, VTMHIP_DCT8 = 1, VTMHIP_DST7 = 2,      /* TransType, CommonLib/TypeDef.h */
       VTMHIP_TRSKIP = 3 };                                    /* fused chain only: the MTS_SKIP candidate (xTransformSkip / xITransformSkip, no transform) */

typedef struct vtmhip_ctx vtmhip_ctx;

/* ---- context ------------------------------------------------------------------------------------------------ */
int         vtmhip_abi_version( void );
int         vtmhip_struct_size( int which );   /* sizeof() of the job/result structs below, in declaration order (0 = vtmhip_dist_job ...): lets a foreign-language binding verify its layout */
int         vtmhip_device_count( int *count );
int         vtmhip_create( int device, vtmhip_ctx **ctx );              /* one context per encoder stack / per rank */
int         vtmhip_destroy( vtmhip_ctx *ctx );
int         vtmhip_set_stream( vtmhip_ctx *ctx, void *hipStream );     /* launch on the caller's hipStream_t; NULL = HIP's default stream (torch's default) */
int         vtmhip_use_own_stream( vtmhip_ctx *ctx );                  /* back to the non-blocking stream the context created (the initial state) */
int         vtmhip_sync( vtmhip_ctx *ctx );                            /* waits for the context's stream */
const char *vtmhip_last_error( vtmhip_ctx *ctx );
const char *vtmhip_status_string( int status );

/* device memory helpers for hosts without their own allocator (the C++ encoder); torch hosts pass data_ptr() */
int vtmhip_dev_alloc( vtmhip_ctx *ctx, size_t bytes, void **devPtr );
int vtmhip_dev_free( vtmhip_ctx *ctx, void *devPtr );
int vtmhip_host_alloc( vtmhip_ctx *ctx, size_t bytes, void **hostPtr );         /* page-locked host memory: job / result slots a hook re-uses for every call (h2d / d2h from it do not stage) */
int vtmhip_host_free( vtmhip_ctx *ctx, void *hostPtr );
int vtmhip_h2d( vtmhip_ctx *ctx, void *dev, const void *host, size_t bytes );   /* asynchronous on the stream */
int vtmhip_d2h( vtmhip_ctx *ctx, void *host, const void *dev, size_t bytes );   /* synchronises before returning */
/* stream timing with HIP events (bench.py uses this around the timed region) */
int vtmhip_timer_start( vtmhip_ctx *ctx );
int vtmhip_timer_stop_ms( vtmhip_ctx *ctx, float *ms );   /* synchronises */

/* per-kernel launch timing: while enabled, every launch of the library's main kernels (tz_search_kernel, full_search_kernel, full_search_sq_kernel,
 * frac_search_sq_kernel, frac_search_kernel, motion_comp_kernel, tu_chain_uni_kernel, tu_ts_kernel, dist_uniform_kernel, satd8_grid_kernel) is
 * bracketed by HIP events on the stream it is launched on.  vtmhip_kernel_timing( ctx, 1 ) clears the record and starts, ( ctx, 0 ) stops;
 * _read synchronises the device and returns the summed duration and the number of launches of one kernel since the start. */
int vtmhip_kernel_timing( vtmhip_ctx *ctx, int enable );
int vtmhip_kernel_timing_read( vtmhip_ctx *ctx, const char *kernel, double *totalMs, int *launches );

/* ================================================================================================================
 * (1) POINTER-SURFACE CALLS -- host pointers
 * ============================================================================================================== */

/* DistParam::distFunc for DF_SAD* / DF_HAD* / DF_SSE* (RdCost.cpp:493-1003, 2819-2934, 1783-2133).
 * org/cur: top-left sample of the W x H blocks, strides in samples.  subShift as DistParam::subShift (SAD only).
 * Any int16 sample values are accepted (bi-pred ME passes 2*org - pred).
 * The reference guards (applyWeight, useMR, step != 1) stay in the trampoline: fall back to the scalar function. */
int vtmhip_xGetSAD( vtmhip_ctx *ctx, const int16_t *org, int orgStride, const int16_t *cur, int curStride, int width, int height, int subShift,
                    uint64_t *dist );
int vtmhip_xGetHADs( vtmhip_ctx *ctx, const int16_t *org, int orgStride, const int16_t *cur, int curStride, int width, int height,
                     uint64_t *dist );
int vtmhip_xGetSSE( vtmhip_ctx *ctx, const int16_t *org, int orgStride, const int16_t *cur, int curStride, int width, int height,
                    uint64_t *dist );
/* DistParam::distFunc for DF_SAD_WITH_MASK (RdCost::xGetSADwMask, RdCost.cpp:3513-3549; set up by the mask overload of setDistParam :3488-3511;
 * GEO merge estimation EncCu.cpp:2930-2960): sum |org - cur| * mask, the mask walked with stepX (+1 / -1) per sample and
 * maskStride * (1 << subShift) + maskStride2 per row, as the scalar reference does. */
int vtmhip_xGetSADwMask( vtmhip_ctx *ctx, const int16_t *org, int orgStride, const int16_t *cur, int curStride, int width, int height, int subShift,
                         const int16_t *mask, int maskStride, int stepX, int maskStride2, uint64_t *dist );


/* InterpolationFilter::m_filterHor / m_filterVer [tapIdx][isFirst][isLast] and m_filterCopy[isFirst][isLast]
 * (InterpolationFilter.h:93-95; filter<> InterpolationFilter.cpp:548-651, filterCopy<> :398-525).  `src` points at the
 * OUTPUT-aligned sample, as in the reference: the callee reads (taps/2 - 1) samples before it along the filter direction.
 * taps: 8, 4 or 2; coeff: `taps` filter taps; clipMin/clipMax/bitDepth: ClpRng::min/max/bd. */
int vtmhip_filterHor( vtmhip_ctx *ctx, int taps, int isFirst, int isLast, const int16_t *src, int srcStride, int16_t *dst, int dstStride, int width,
                      int height, const int16_t *coeff, int bitDepth, int clipMin, int clipMax, int biMCForDMVR );
int vtmhip_filterVer( vtmhip_ctx *ctx, int taps, int isFirst, int isLast, const int16_t *src, int srcStride, int16_t *dst, int dstStride, int width,
                      int height, const int16_t *coeff, int bitDepth, int clipMin, int clipMax, int biMCForDMVR );
int vtmhip_filterCopy( vtmhip_ctx *ctx, int isFirst, int isLast, const int16_t *src, int srcStride, int16_t *dst, int dstStride, int width, int height,
                       int bitDepth, int clipMin, int clipMax, int biMCForDMVR );

/* fastFwdTrans[type][log2(n)-1] / fastInvTrans[type][log2(n)-1] (TrQuant.cpp:69-81; typedefs TrQuant.h:53-54): 1-D transform of `line`
 * rows, TRANSPOSED output dst[k*line + j] (forward) / dst[i*n + j] (inverse), zero-out through skipLine / skipLine2.
 * (type, n) pairs whose table slot is nullptr in the reference return VTMHIP_E_INVALID. */
int vtmhip_fastFwdTrans( vtmhip_ctx *ctx, int type, int n, const int32_t *src, int32_t *dst, int shift, int line, int skipLine, int skipLine2 );
int vtmhip_fastInvTrans( vtmhip_ctx *ctx, int type, int n, const int32_t *src, int32_t *dst, int shift, int line, int skipLine, int skipLine2,
                         int32_t outputMinimum, int32_t outputMaximum );
/* LFNST kernels: TrQuant::fwdLfnstNxN / invLfnstNxN (TrQuant.cpp:233-311; called by xFwdLfnst / xInvLfnst :313-527, which gather / scatter the
 * low-frequency region on the host).  The trained core matrices g_lfnst8x8[4][2][16][48] and g_lfnst4x4[4][2][16][16] (Rom.h:132-133, int8) are the
 * CALLER's data: the integration hands the reference's own arrays over once per context; nothing of them is compiled into this library.
 * forward: dst[j] = ( sum_i src[i] * M[j][i] + 64 ) >> 7 for j < zeroOutSize, zeros up to trSize (16 / 48);
 * inverse: dst[j] = clip( ( sum_{i < zeroOutSize} src[i] * M[i][j] + 64 ) >> 7, +-2^15 ) for j < trSize.   size: 4 or 8 (the `size > 4` switch). */
int vtmhip_lfnst_set_tables( vtmhip_ctx *ctx, const int8_t *lfnst8x8, const int8_t *lfnst4x4 );
int vtmhip_fwdLfnstNxN( vtmhip_ctx *ctx, const int32_t *src, int32_t *dst, int mode, int index, int size, int zeroOutSize );
int vtmhip_invLfnstNxN( vtmhip_ctx *ctx, const int32_t *src, int32_t *dst, int mode, int index, int size, int zeroOutSize );
typedef struct
{
  int64_t srcOff, dstOff;       /* coefficients inside d_srcBase / d_dstBase: forward reads trSize and writes trSize, inverse reads zeroOutSize and writes trSize */
  uint8_t mode, index;          /* g_lfnstLut[intraMode] (0..3), lfnstIdx - 1 (0..1) */
  uint8_t size;                 /* 4: the 16 x 16 matrices, 8: the 16 x 48 ones */
  uint8_t zeroOutSize;          /* 8 or 16 */
  uint8_t inverse, pad0, pad1, pad2;
} vtmhip_lfnst_job;
int vtmhip_lfnst_batch_dev( vtmhip_ctx *ctx, const int32_t *d_srcBase, int32_t *d_dstBase, const vtmhip_lfnst_job *d_jobs, int n );

/* The whole secondary transform of a TU, TrQuant::xFwdLfnst / xInvLfnst (TrQuant.cpp:340-527), IN PLACE on its W x H coefficient block (stride W):
 * gather of the low-frequency region (transposed for the intra modes past the diagonal, getTransposeFlag :334-338), the core multiply above, scatter along
 * the coefficient scan (forward: 16 / 48 positions; inverse: gather 16 scan positions, write the 16 / 48 region samples).  The trampoline derives
 * mode = g_lfnstLut[ getLFNSTIntraMode( PU::getWideAngle( ... ) ) ] and transpose from the PU exactly as the reference does (:350-366, 438-454). */
typedef struct
{
  int64_t coefOff;          /* the TU's coefficients inside d_coefBase */
  int16_t width, height;    /* 4..64 */
  uint8_t mode, index;      /* g_lfnstLut[intraMode] (0..3), lfnstIdx - 1 (0..1) */
  uint8_t transpose, inverse;
} vtmhip_lfnst_tu_job;
int vtmhip_lfnst_tu_batch_dev( vtmhip_ctx *ctx, int32_t *d_coefBase, const vtmhip_lfnst_tu_job *d_jobs, int n );
/* host-only: the scan positions (x + y * width) the calls above use, 16 (4-wide / 4-high TUs) or 48 entries */
int vtmhip_lfnst_scan_host( int width, int height, int32_t *pos48 );

/* n x n forward core matrix g_trCore<type>P<n>[TRANSFORM_FORWARD] (Rom.h:115-130), row-major int16; host-only helper */
int vtmhip_tr_matrix_host( int type, int n, int16_t *out );
/* MTS candidate pre-selection thresholds of TrQuant::transformNxN( tu, compID, cQP, &trModes, maxCand ) (TrQuant.cpp:950-1019); host-only */
int vtmhip_mts_select( const int32_t *sumAbs, int numCand, int width, int height, int maxCand, uint8_t *test );
/* the same from RAW sums with the transform-skip scaling of :992-1001 applied here: mtsIdx[i] = the candidate's tu.mtsIdx (MTS_SKIP = 1 marks
 * sum |residual| of a transform-skip candidate); maxLog2TrDynamicRange: sps.getMaxLog2TrDynamicRange() (15).  numCand <= 16. */
int vtmhip_mts_select2( const int32_t *sumAbs, const uint8_t *mtsIdx, int numCand, int width, int height, int bitDepth, int maxLog2TrDynamicRange,
                        int maxCand, uint8_t *test );

/* ================================================================================================================
 * (2) BATCHED DEVICE CALLS -- device pointers, asynchronous on the context's stream
 *     One exception to "asynchronous": a MIXED-shape batch (no uniform promise) of >= 64 jobs to vtmhip_xMotionEstimation_batch_dev or >= 256 jobs to
 *     vtmhip_tu_chain_batch_dev is bucketed by block shape on the device, and the class counts (80 bytes) are read back with ONE
 *     hipStreamSynchronize inside the call.  While the stream is being captured into a hipGraph the bucketing is skipped (the generic chain runs the
 *     whole batch: same results); uniform batches never synchronise.
 * ============================================================================================================== */

/* One distortion evaluation: org block at orgBase + orgOff, candidate block at curBase + curOff (offsets in samples). */
typedef struct
{
  int64_t orgOff;
  int64_t curOff;
  int32_t orgStride;
  int32_t curStride;
  int16_t width;
  int16_t height;
  int16_t subShift;   /* SAD only */
  int16_t kind;       /* VTMHIP_DIST_* */
} vtmhip_dist_job;

/* n independent distFunc evaluations (hooks B1-B7, B10).  d_jobs and d_dist are device arrays of n entries. */
int vtmhip_dist_batch_dev( vtmhip_ctx *ctx, const int16_t *d_orgBase, const int16_t *d_curBase, const vtmhip_dist_job *d_jobs, int n,
                           uint64_t *d_dist );

typedef struct
{
  int64_t orgOff, curOff, maskOff;   /* maskOff: first mask sample (DistParam::mask) inside d_maskBase */
  int32_t orgStride, curStride, maskStride, maskStride2;
  int16_t width, height, subShift, stepX;
} vtmhip_masked_sad_job;

/* n masked SADs (DF_SAD_WITH_MASK), e.g. every (GEO split, merge candidate) pair of a CU in one launch */
int vtmhip_masked_sad_batch_dev( vtmhip_ctx *ctx, const int16_t *d_orgBase, const int16_t *d_curBase, const int16_t *d_maskBase,
                                 const vtmhip_masked_sad_job *d_jobs, int n, uint64_t *d_dist );

/* The same distortions for a batch the caller promises to be uniform: EVERY job is width x height of one `kind` (and subShift for SAD); the jobs'
 * own width / height / kind / subShift fields are ignored.  Small blocks then share a wave (an 8x8 SATD is one Hadamard tile = one lane): the form
 * hooks B7 / B10 use for the merge / AMVP candidates of one CU size. */
int vtmhip_dist_uniform_batch_dev( vtmhip_ctx *ctx, const int16_t *d_orgBase, const int16_t *d_curBase, const vtmhip_dist_job *d_jobs, int n,
                                   int kind, int width, int height, int subShift, uint64_t *d_dist );

/* Intra mode pre-selection (IntraSearch::estIntraPredLumaQT, EncoderLib/IntraSearch.cpp:555-592: per tested mode `min( 2 * SAD, SATD )` of the mode's prediction against
 * the original block -- the same DistParam::distFunc slots as the inter path): the N candidate predictions of ONE block in one call.  The host forms the predictors
 * (predIntraAng: angular / planar / DC with PDPC, reference smoothing -- not part of this library) as N consecutive width x height blocks (stride = width) at d_predBase +
 * predOff; the original block sits at d_orgBase + orgOff.  d_dist[0 .. N) = the SADs, d_dist[N .. 2N) = the SATDs (xGetHADs tile rules), in candidate order. */
int vtmhip_intra_cand_cost_batch_dev( vtmhip_ctx *ctx, const int16_t *d_orgBase, int64_t orgOff, int orgStride, const int16_t *d_predBase, int64_t predOff, int n, int width,
                                      int height, uint64_t *d_dist );

/* ---- luma-level-weighted SSE: RdCost::m_afpDistortFunc[DF_SSE_WTD .. DF_SSE16N_WTD] (RdCost::xGetSSE*_WTD, CommonLib/RdCost.cpp:3088-3463; slots :190-197;
 * per-sample rule RdCost::getWeightedMSE :3055-3086) -- the CU-level final distortion with LMCS (LMCSEnable) or the luma-level-to-delta-QP (WCG) mode on:
 * InterSearch::encodeResAndCalcRdInterCU (EncoderLib/InterSearch.cpp:7247-7264, 7585-7596), EncCu's skip / merge reconstruction distortion
 * (EncCu.cpp:4180-4184, 4687-4690), the intra RD loops (IntraSearch.cpp:1711, 3299-3306, 4631-4742).  Per sample of a W x H block (x < W, y < H):
 *   d      = org - cur
 *   lumaLv = Y: org;  Cb / Cr: orgLuma[(x << cShiftX) + (y << cShiftY) * orgLumaStride]
 *   w      = Y: LUT[lumaLv];  Cb / Cr: signalType SDR (0) / HLG (2) ? chromaWeight : LUT[lumaLv]
 *   mse    = (int32_t) ( ( (int64_t) ( w * 65536.0 ) * ( d * d ) + 32768 ) >> 16 )        (Intermediate_Int is int: TRUNCATED to 32 bits)
 *   dist  += (uint64_t) (int64_t) mse                                                        (DISTORTION_PRECISION_ADJUSTMENT = 0, FULL_NBIT)
 * Sample contract: org, cur and orgLuma in [0, 2^bitDepth), bitDepth <= 12 (the reference CHECKs org >= 0; |d| < 2^12 keeps d * d < 2^24).
 * The tables are the host's (RdCost::m_reshapeLumaLevelToWeightPLUT, m_chromaWeight, m_signalType; EncGOP.cpp:228-234, 1810-1853); the chroma
 * m_distortionWeight scaling of RdCost::getDistPart (:411-455) stays with the caller, as for DF_SSE.  applyWeight (RdCostWeightPrediction::xGetSSEw) is
 * not this entry: vtmhip_xGetSSEw below. */

/* The weight tables of a context: lut[1 << lumaBD] = m_reshapeLumaLevelToWeightPLUT, converted here to the reference's fixed point (int64_t)( w * 65536.0 );
 * every converted weight (and chromaWeight's) must lie in [0, 2^31) or the call fails.  invLut: the reshaper's inverse LUT (Reshape::getInvLUT(), 1 << lumaBD
 * entries) for VTMHIP_WTD_INV_RESHAPE_CUR jobs, or NULL.  lumaBD: 8..12.  The copies are ordered on the context's stream before every later launch and done
 * when the call returns (the caller may free its arrays).  Call it after RdCost::initLumaLevelToWeightTableReshape() and after every updateReshape... /
 * restore... of EncGOP.cpp:1810-1853.  Every DF_SSE_WTD entry fails with VTMHIP_E_INVALID until it has been called. */
int vtmhip_set_luma_level_weights( vtmhip_ctx *ctx, const double *lut, int lumaBD, int signalType, double chromaWeight, const int16_t *invLut );

/* DistParam::distFunc for all eight DF_SSE*_WTD slots (host pointers, like vtmhip_xGetSSE).  compID: 0 = Y, 1 = Cb, 2 = Cr; cShiftX / cShiftY: 0 or 1
 * (getComponentScaleX / Y of the chroma format; 0 for Y).  orgLuma / orgLumaStride: DistParam::orgLuma of a chroma block (the co-located luma original);
 * ignored for Y, whose weight index is org itself (the reference CHECKs orgLuma == org).  A negative org sample is VTMHIP_E_INVALID (the reference's CHECK). */
int vtmhip_xGetSSE_WTD( vtmhip_ctx *ctx, const int16_t *org, int orgStride, const int16_t *cur, int curStride, int width, int height, int compID,
                        const int16_t *orgLuma, int orgLumaStride, int cShiftX, int cShiftY, uint64_t *dist );

#define VTMHIP_WTD_INV_RESHAPE_CUR 1   /* map cur through the inverse LUT first: tmpRecLuma.rspSignal( m_pcReshape->getInvLUT() ) (Buffer.cpp:400-413), Y only */
#define VTMHIP_WTD_INVALID_DIST    UINT64_MAX   /* d_dist of a job the kernel rejected (see vtmhip_sse_wtd_batch_dev) */
typedef struct
{
  int64_t orgOff, curOff, orgLumaOff;          /* samples inside d_orgBase / d_curBase / d_orgLumaBase (orgLumaOff: chroma jobs only) */
  int32_t orgStride, curStride, orgLumaStride;
  int16_t width, height;                       /* 1..128 */
  uint8_t compID, cShiftX, cShiftY, flags;     /* flags: VTMHIP_WTD_* */
  int32_t pad;
} vtmhip_wtd_job;

/* n DF_SSE*_WTD evaluations in one launch, e.g. the Y, Cb and Cr final distortions of every CU of a level; d_dist[i] = the raw distFunc value (the
 * caller applies m_distortionWeight to chroma, as with vtmhip_dist_batch_dev).  Small blocks share a wave (their row segments are spread over its lanes).
 * The jobs are device-resident, so a job the kernel cannot evaluate -- width / height outside 1..128, compID > 2, a cShift > 1 or a Y job with a cShift,
 * unknown flags, VTMHIP_WTD_INV_RESHAPE_CUR on chroma or without an inverse LUT -- gets d_dist = VTMHIP_WTD_INVALID_DIST and is not read; the call itself
 * fails only on what the host can see (no table set, null pointers). */
int vtmhip_sse_wtd_batch_dev( vtmhip_ctx *ctx, const int16_t *d_orgBase, const int16_t *d_curBase, const int16_t *d_orgLumaBase, const vtmhip_wtd_job *d_jobs,
                              int n, uint64_t *d_dist );

/* ---- explicit weighted prediction (WeightedPredP / WeightedPredB): the distortion and sample ops of a weighted-prediction slice ------------------------
 * Distortion: with DistParam::applyWeight every SAD / HAD / SSE / SSE_WTD slot hands off to RdCostWeightPrediction::xGetSADw / xGetHADsw / xGetSSEw
 * (CommonLib/RdCost.cpp:495, 532, ..., 2821, 3090-3374; CommonLib/RdCostWeightPrediction.cpp:56-640), with the U0040_... = 1 branches (TypeDef.h:164).
 * Motion estimation sets the flag and DistParam::wpCur in InterSearch::setWpScalingDistParam (EncoderLib/InterSearch.cpp:6057-6098, called at :3377).
 * vtmhip_wp_param = the derived fields w, offset, shift, round of the block's component's WPScalingParam (Slice.h:2206-2222).  Per sample, q = ((w * cur +
 * round) >> shift) + offset (arithmetic shift), Pel(v) = v truncated to int16, clip(v) = min(max(v, 0), 2^bitDepth - 1):
 *   SADw  w == 1 << shift: offset == 0: |org - cur|;  bi: |org - (cur + offset)| (int, no clip, no Pel);  uni: |org - clip(cur + offset)|
 *         otherwise:       bi: |org - Pel(q)|;  uni: |org - clip(q)|
 *         after each row, if maxDist < sum the running sum is returned (the early exit: a PREFIX of the rows, not the whole block); subShift is ignored
 *         (every row is read), so the entries take none
 *   SSEw  residual = Pel(org - pred), pred = bi ? Pel(q) : clip(q);  sum += residual^2 (uint64); no early exit.  A nonzero subShift is the reference's CHECK.
 *   HADsw diff = org - Pel(q) (never clipped, uni or bi; TCoeff).  W % 8 == 0 and H % 8 == 0: 8x8 Hadamard tiles, each (s + 2) >> 2 (no 8x16 / 16x8 tiles
 *         and no DC adjustment, unlike xGetHADs); else W % 4 == 0 and H % 4 == 0: 4x4 tiles, (s + 1) >> 1; else 2x2 tiles, not normalised, in the reference's
 *         row walk: the y += 2 loop advances org / cur by ONE row, so step k reads rows k and k + 1 (:624-633).  step is 1 (step != 1 stays on the host).
 *   DISTORTION_PRECISION_ADJUSTMENT is 0 (FULL_NBIT, TypeDef.h:225-237): no final shift.
 * Sample contract: bitDepth 8..12; w in [-256, 256], shift 0..8, offset and round in [-32768, 32767] (the reference derives |w| <= 255, shift <= 8); HAD
 * blocks on the 2x2 path have even W and H (odd ones read outside the block in the reference); width / height 1..128.  Anything else is VTMHIP_E_INVALID
 * (pointer entries) or VTMHIP_WP_INVALID_DIST (batched). */
typedef struct
{
  int32_t w, offset, shift, round;   /* WPScalingParam::w / offset / shift / round of one component */
} vtmhip_wp_param;

/* DistParam::distFunc of the SAD / HAD / SSE (and SSE_WTD) slots under applyWeight (host pointers, like vtmhip_xGetSAD).  wp: &DistParam::wpCur[compID];
 * isBiPred: DistParam::isBiPred; maxDist: DistParam::maximumDistortionForEarlyExit (SADw only). */
int vtmhip_xGetSADw( vtmhip_ctx *ctx, const int16_t *org, int orgStride, const int16_t *cur, int curStride, int width, int height, const vtmhip_wp_param *wp,
                     int bitDepth, int isBiPred, uint64_t maxDist, uint64_t *dist );
int vtmhip_xGetSSEw( vtmhip_ctx *ctx, const int16_t *org, int orgStride, const int16_t *cur, int curStride, int width, int height, const vtmhip_wp_param *wp,
                     int bitDepth, int isBiPred, uint64_t *dist );
int vtmhip_xGetHADsw( vtmhip_ctx *ctx, const int16_t *org, int orgStride, const int16_t *cur, int curStride, int width, int height, const vtmhip_wp_param *wp,
                      int bitDepth, int isBiPred, uint64_t *dist );

#define VTMHIP_WP_INVALID_DIST UINT64_MAX   /* d_dist of a job the kernel rejected (see vtmhip_wp_dist_batch_dev) */
typedef struct
{
  int64_t         orgOff, curOff;          /* samples inside d_orgBase / d_curBase */
  int32_t         orgStride, curStride;
  int16_t         width, height;           /* 1..128 */
  uint8_t         kind;                    /* VTMHIP_DIST_SAD (xGetSADw), VTMHIP_DIST_SATD (xGetHADsw), VTMHIP_DIST_SSE (xGetSSEw) */
  uint8_t         bitDepth, isBiPred, pad;
  vtmhip_wp_param wp;
  uint64_t        maxDist;                 /* SAD only: maximumDistortionForEarlyExit (UINT64_MAX: no early exit) */
} vtmhip_wp_dist_job;

/* n weighted distortions in one launch; d_dist[i] = the distFunc value.  Small blocks share a wave.  The jobs are device-resident, so a job outside the
 * sample contract above (or with an unknown kind / isBiPred > 1) gets d_dist = VTMHIP_WP_INVALID_DIST and is not read; the call itself fails only on what
 * the host can see (null pointers, n < 0). */
int vtmhip_wp_dist_batch_dev( vtmhip_ctx *ctx, const int16_t *d_orgBase, const int16_t *d_curBase, const vtmhip_wp_dist_job *d_jobs, int n, uint64_t *d_dist );

/* Sample ops: WeightPrediction::addWeightUni / addWeightBi (CommonLib/WeightPrediction.cpp:46-64, 157-226, 288-392), called from
 * InterPrediction::motionCompensation (InterPrediction.cpp:633, 639) and the bi-pred ME target preparation (InterSearch.cpp:3261, 3286).  Inputs are the
 * 14-bit intermediates vtmhip_mc_batch_dev writes with bi = 1 (a weighted-prediction PU is two launches).  With shiftNum = IF_INTERNAL_FRAC_BITS(bd) =
 * max(2, 14 - bd) (JVET_R0351_HIGH_BIT_DEPTH_SUPPORT = 1, TypeDef.h:59; InterpolationFilter.h:54) and P' = P + 8192 (IF_INTERNAL_OFFS):
 *   bi (weightBidir):   s = shift + shiftNum;  dst = clip( (w0 * P0' + w1 * P1' + (1 << (s - 1)) + (offset << (s - 1))) >> s )   (bRoundLuma = true)
 *   uni, w0 != 1 << shift (weightUnidir):                     s = shift + shiftNum;  dst = clip( ((w0 * P0' + (1 << (s - 1))) >> s) + offset )
 *   uni, w0 == 1 << shift (noWeightUnidir / noWeightOffsetUnidir):  dst = clip( ((P0' + (1 << (shiftNum - 1))) >> shiftNum) + offset )
 * The job carries the WPScalingParam fields as WeightPrediction::getWpScaling leaves them (:77-155), with o = iOffset << (bitDepth - 8) (1 with high-precision
 * offsets):  uni: w0 = iWeight, offset = o, shift = log2Denom, round = log2Denom >= 1 ? 1 << (log2Denom - 1) : 0;  bi: w0 = iWeight of list 0, w1 = iWeight
 * of list 1, offset = o0 + o1, shift = log2Denom + 1, round = 1 << log2Denom.  The ops derive their own rounding from shift, so `round` is not read (as in
 * the reference).  Sample contract as above (w0 / w1 in [-256, 256], shift 0..8, offset in [-32768, 32767], bitDepth 8..12, width / height 1..128); a job
 * outside it leaves its dst block untouched. */
enum { VTMHIP_WP_UNI = 0, VTMHIP_WP_BI = 1 };
typedef struct
{
  int64_t src0Off, src1Off, dstOff;        /* samples inside d_src0Base / d_src1Base / d_dstBase (src1: VTMHIP_WP_BI only) */
  int32_t src0Stride, src1Stride, dstStride;
  int16_t width, height;
  uint8_t bitDepth, mode, pad0, pad1;      /* mode: VTMHIP_WP_UNI / VTMHIP_WP_BI */
  int32_t w0, w1, offset, shift, round;
} vtmhip_wp_pred_job;

int vtmhip_wp_pred_batch_dev( vtmhip_ctx *ctx, const int16_t *d_src0Base, const int16_t *d_src1Base, int16_t *d_dstBase, const vtmhip_wp_pred_job *d_jobs, int n );

/* SATD 8x8 block-grid micro-benchmark: every 8-aligned 8x8 block of the W x H org picture against the
 * reference picture displaced by (dx,dy) in [-r,r]^2.  d_ref must carry >= r samples of valid margin on every side.
 * d_dist[(by*(W/8)+bx)*(2r+1)^2 + (dy+r)*(2r+1) + (dx+r)], 32-bit (an 8x8 SATD of int16 samples fits). */
int vtmhip_satd8_grid_dev( vtmhip_ctx *ctx, const int16_t *d_org, int orgStride, const int16_t *d_ref, int refStride, int width, int height,
                           int r, uint32_t *d_dist );

/* ---- reference planes under d_refBase: what must be readable ---------------------------------------------------------
 * A reference plane handed to any *_dev call is the reconstructed picture WITH its border: at least ctuSize + 16 samples on every side (the reference's own
 * Picture::margin, 144 for CTU 128: clipMv keeps a block's origin inside [-ctuSize - 7, pic + 7], the 8-tap filter adds 3 / 4 samples, the block its size).
 * The kernels fetch reference samples in whole 16-byte groups and whole window rows (search windows, the column-walking raster scan), so a fetch may start
 * before / end after the samples it uses: the library may READ (never write, never use) up to VTMHIP_PLANE_SLACK samples before the first and after the last
 * sample of a plane (first = row -margin, column -margin; last = the last sample of row height + margin - 1).  Planes that sit inside one allocation (the DPB
 * layout of DESIGN.md section 2) give each other that slack; the first and the last plane of an allocation need VTMHIP_PLANE_SLACK readable samples in front
 * of / behind them -- allocate ( samples + 2 * VTMHIP_PLANE_SLACK ) and hand over the pointer VTMHIP_PLANE_SLACK samples in (oracle/ref_shim_enc.cpp:refPlane
 * does exactly that for the encoder's pictures; tests/pis_golden.py:build_dpb for the recorded planes). */
#define VTMHIP_PLANE_SLACK 2048

/* ---- integer motion search ----------------------------------------------------------------------------------- */
typedef struct
{
  int32_t picW, picH;   /* pps.getPicWidth/HeightInLumaSamples: clipMv / xClipMv limits */
  int32_t ctuSize;      /* sps.getMaxCUWidth() */
  int32_t bitDepth;     /* sps.getBitDepth( CHANNEL_TYPE_LUMA ): 8 .. 12 (the library's sample contract); every entry that takes these parameters returns VTMHIP_E_INVALID outside it */
  int32_t wavesPerJob;  /* tuning hint for this batch: 0/1 = one wave per search; 2, 4, 8, 16 = waves that split each candidate list (large PUs) */
  int32_t maxSearchRange; /* tuning hint: the largest searchRange of the batch's TZ jobs (m_aaiAdaptSR: up to 384 with ASR).  The raster scan of xTZSearch (:3888-3899) is run by a
                             column-walking kernel whose per-scan totals live in LDS: 0 (or <= 96) sizes it for the 39 x 39 points of SearchRange 96; a larger value for
                             ((2 * range) / 5 + 1)^2 points (384: 154 x 154), capped at what one CU's LDS holds (201 x 201 points = range 500).  A scan that does not fit runs
                             inside the search kernel: same result, much slower.  Any value is accepted (a hint never makes a call fail). */
} vtmhip_pic_params;

/* One (PU, reference picture) integer search = one call of InterSearch::xTZSearch. */
typedef struct
{
  int64_t orgOff;       /* sample offset of the PU's top-left in the original plane (pcPatternKey)         */
  int64_t refOff;       /* sample offset of the SAME position (MV 0,0) in the reference plane (piRefY)      */
  int32_t orgStride, refStride;
  int16_t puX, puY;     /* luma position of the PU in the picture                                          */
  int16_t width, height;
  int16_t subShift;     /* DistParam::subShift after setDistParam(subShiftMode) (RdCost.cpp:289-323)       */
  uint8_t imvShift;
  uint8_t signedSamples;   /* 0: every org/ref sample is >= 0 (uni-pred ME on pictures); 1: full int16 range (2*org - pred targets) */
  int32_t predHor, predVer;     /* RdCost::setPredictor, quarter-sample units                              */
  double  motionLambda;         /* RdCost::m_motionLambda                                                  */
  int32_t mvHor, mvVer;         /* rcMv on entry (internal 1/16 precision)                                 */
  int32_t searchRange;          /* m_iSearchRange                                                          */
  uint8_t extendedSettings, fastSettings, firstSearchStop, hasIntMv2Nx2NPred;
  int32_t intMv2Nx2NPredHor, intMv2Nx2NPredVer;
  int32_t numExtraStart;        /* m_uniMvList candidates, de-duplicated by the caller (InterSearch.cpp:3728-3746) */
  int32_t extraStart[15][2];    /* internal precision */
} vtmhip_tz_job;

typedef struct
{
  int32_t  mvX, mvY;   /* integer MV (rcMv on return) */
  uint32_t nEval;      /* distFunc evaluations performed (statistics; the reference does not return it) */
  uint32_t reserved;
  uint64_t cost;       /* cStruct.uiBestSad: distortion + MV rate */
  uint64_t dist;       /* ruiSAD */
} vtmhip_me_result;

int vtmhip_tz_search_batch_dev( vtmhip_ctx *ctx, const vtmhip_pic_params *pic, const int16_t *d_orgBase, const int16_t *d_refBase,
                                const vtmhip_tz_job *d_jobs, int n, vtmhip_me_result *d_results );


/* One exhaustive search = xSetSearchRange + xPatternSearch (InterSearch.cpp:3496-3608): every integer position of the
 * clipped window around `center`, first strict minimum in raster order (hook B5, the +-BipredSearchRange refinement). */
typedef struct
{
  int64_t orgOff, refOff;
  int32_t orgStride, refStride;
  int16_t puX, puY, width, height;
  int16_t subShift;
  uint8_t imvShift;
  uint8_t signedSamples;        /* 1 for the bi-pred target 2*org - pred */
  int32_t predHor, predVer;     /* quarter-sample units */
  double  motionLambda;
  int32_t centerHor, centerVer; /* bestInitMv, internal 1/16 precision */
  int32_t searchRange;          /* iSrchRng (BipredSearchRange = 4) */
  int32_t pad;
} vtmhip_full_job;

int vtmhip_full_search_batch_dev( vtmhip_ctx *ctx, const vtmhip_pic_params *pic, const int16_t *d_orgBase, const int16_t *d_refBase,
                                  const vtmhip_full_job *d_jobs, int n, vtmhip_me_result *d_results );
/* Same searches, same results, for a batch the caller promises to be uniform: EVERY job is width x height with searchRange <= 4
 * (the bi-pred refinement of one quadtree level or of one split shape).  Squares 8 .. 64 and the binary / ternary split shapes 16x8, 32x8, 32x16, 64x16,
 * 64x32 in both orientations: one lane per candidate over an LDS-resident window; any other shape forwards to vtmhip_full_search_batch_dev.
 * The reference plane must be readable 7 samples beyond the search window's right edge. */
int vtmhip_full_search_uniform_batch_dev( vtmhip_ctx *ctx, const vtmhip_pic_params *pic, const int16_t *d_orgBase, const int16_t *d_refBase,
                                          const vtmhip_full_job *d_jobs, int n, int width, int height, vtmhip_me_result *d_results );
/* width == height == size */
int vtmhip_full_search_square_batch_dev( vtmhip_ctx *ctx, const vtmhip_pic_params *pic, const int16_t *d_orgBase, const int16_t *d_refBase,
                                         const vtmhip_full_job *d_jobs, int n, int size, vtmhip_me_result *d_results );

/* ---- whole motion estimation of one (PU, list, refIdx): InterSearch::xMotionEstimation -------------------------------------
 * (InterSearch.cpp:3299-3494; AMVR integer refinement xPatternSearchIntRefine :4172-4282).  One call runs, for n jobs:
 *   bi:  pattern = 2*org - otherPred (removeHighFreq :3320-3326), best start among rcMv and the m_uniMvList entries (:3377-3420),
 *        xSetSearchRange + xPatternSearch over +-bipredSearchRange;        uni: xTZSearch from rcMvPred (:3440-3446)
 *   cu.imv 0 / IMV_HPEL: xPatternSearchFracDIF and the rate re-weighting of :3478-3484
 *   cu.imv 1 / 2:        xPatternSearchIntRefine over 9 positions x the AMVP candidates
 * as a fixed sequence of launches on the context's stream (no host synchronisation).  Not covered (the trampoline keeps the host
 * path): BCW weights, weighted prediction, MCTS, composite references, the block-MV cache (xReadBufferedUniMv / CacheBlkInfoCtrl). */
typedef struct
{
  int32_t bipredSearchRange;       /* m_bipredSearchRange */
  uint8_t useHadME;                /* HadamardME && !slice.getDisableSATDForRD() */
  uint8_t fastInterSearchMode13;   /* FEN mode 1 or 3: setDistParam subShiftMode 2 (RdCost.cpp:289-323); else 0 */
  uint8_t extendedSettings;        /* MESEARCH_DIAMOND_ENHANCED */
  uint8_t firstSearchStop;         /* FastMEAssumingSmootherMVEnabled */
  int32_t uniformImv;              /* -1: jobs mix cu.imv values; 0..3: every job of the batch has this cu.imv (lets whole stages be skipped) */
  int32_t uniformSquare;           /* != 0: every job is exactly maxWidth x maxHeight (squares 8 .. 128 or a split shape 16x8 .. 64x32, either orientation:
                                      tiled fractional kernel when uniformImv is 0 or 3); the name predates the rectangular fast paths */
  int32_t uniformBi;               /* 0: jobs mix bBi values; 1: every job is a uni search (no pattern copies: the searches read the original plane);
                                      2: every job is a bi search (no TZ stage; lane-per-candidate exhaustive kernel when uniformSquare) */
  uint8_t noUniMvList;             /* caller's promise: numExtraStart == 0 in every job (with uniformBi 2 the start-candidate SADs are skipped: rcMv is the start) */
  uint8_t biPatternGiven;          /* with uniformBi 2: d_otherPredBase + otherPredOff already holds the search pattern 2*org - otherPred (a fused
                                      vtmhip_motion_compensation_batch_dev epilogue wrote it), not the other list's prediction: no removeHighFreq pass here */
  uint8_t pad0, pad1;
} vtmhip_me_cfg;

typedef struct
{
  int64_t  orgOff, refOff;          /* PU top-left in the original plane / the same position (MV 0,0) in the reference plane */
  int64_t  otherPredOff;            /* bi: block of the other list's prediction inside d_otherPredBase (m_tmpPredStorage[1 - list]) */
  int32_t  orgStride, refStride, otherPredStride;
  int16_t  puX, puY, width, height;
  uint8_t  bi, imv, mvpIdx, numAmvpCand;   /* bBi, cu.imv (0 quarter, 1 integer, 2 four-sample, 3 half), riMVPIdx, amvpInfo.numCand */
  int32_t  mvPredHor, mvPredVer;    /* rcMvPred, internal 1/16 precision */
  int32_t  mvHor, mvVer;            /* rcMv on entry (start of the bi-pred search) */
  int32_t  amvpCand[2][2];          /* amvpInfo.mvCand */
  uint32_t mvpIdxBits[2];           /* m_auiMVPIdxCost[i][AMVP_MAX_NUM_CANDS] */
  uint32_t bits;                    /* ruiBits on entry */
  int32_t  searchRange;             /* m_aaiAdaptSR[list][refIdx] */
  double   motionLambda;
  int32_t  numExtraStart;           /* m_uniMvListSize */
  int32_t  extraStart[15][2];       /* uniMvs[list][refIdx] of the m_uniMvList entries, newest first, duplicates allowed */
  uint32_t flags;                   /* VTMHIP_MEJ_* */
} vtmhip_me_job;
/* uni job: the block-vector cache of the mode control holds an integer vector for this (block, list, refIdx) (CacheBlkInfoCtrl::getMv, InterSearch.cpp:3360-3368):
 * rcMv = mvHor / mvVer (that vector in internal precision) and xTZSearch runs with bFastSettings (:3434-3441) instead of starting at rcMvPred */
#define VTMHIP_MEJ_CACHED_INT_MV 1u
/* uni row of vtmhip_predInterSearch_batch_dev that is GIVEN, not searched (InterSearch::xReadBufferedUniMv :7677-7697: a CU-level BCW weight other than the default re-uses the
 * vectors the default-weight pass left in m_uniMotions): on entry uniOut[row].mvHor / mvVer = the buffered vector and uniOut[row].cost = its distortion WITHOUT any rate; the
 * row's AMVP estimation runs as usual, its bits become the entry bits + the vector's bits against the chosen predictor (both in the AMVR precision) and its cost
 * distortion + getCost( bits ); uniOut[row] then holds that result.  The level lists the (list, refIdx) groups whose rows are all given in vtmhip_pis_level::givenRows. */
#define VTMHIP_MEJ_GIVEN_UNI 2u
/* bi job: flags bits 8..15 = getBcwWeight( cu.BcwIdx, searched list ) as int8 (0 or 4: the default weight): the search target is removeWeightHighFreq( org, otherPred, w )
 * = ( org * w0 - otherPred * w1 + 2^15 ) >> 16 (Buffer.h:417-460) instead of 2 * org - otherPred, and the distortion weight of :3483 / xPatternSearchIntRefine is |w| / 8
 * (xGetMEDistortionWeight :7666-7676) instead of 0.5 */
#define VTMHIP_MEJ_BCW_WEIGHT( flags ) ( ( int ) ( int8_t ) ( ( ( flags ) >> 8 ) & 0xffu ) )
#define VTMHIP_MEJ_BCW_FLAGS( weight ) ( ( ( uint32_t ) ( uint8_t ) ( int8_t ) ( weight ) ) << 8 )

typedef struct
{
  int32_t  mvHor, mvVer;            /* rcMv, internal precision */
  int32_t  mvPredHor, mvPredVer;    /* rcMvPred (changes only in the AMVR integer refinement) */
  int32_t  mvpIdx;                  /* riMVPIdx */
  uint32_t bits;                    /* ruiBits */
  uint64_t cost;                    /* ruiCost */
  int32_t  intX, intY;              /* integer-stage vector (m_integerMv2Nx2N for uni searches) */
  uint64_t intDist;                 /* distortion of the integer stage without the vector rate (the D_ME trace value MECostFPel) */
} vtmhip_me_out;

int vtmhip_xMotionEstimation_batch_dev( vtmhip_ctx *ctx, const vtmhip_pic_params *pic, const vtmhip_me_cfg *cfg, const int16_t *d_orgBase,
                                        const int16_t *d_refBase, const int16_t *d_otherPredBase, const vtmhip_me_job *d_jobs, int n,
                                        int maxWidth, int maxHeight, vtmhip_me_out *d_results );

/* ---- AMVP predictor estimation: InterSearch::xEstimateMvPredAMVP with xGetTemplateCost (hook B7) ----------------------------------
 * (InterSearch.cpp:3088-3128, 3235-3270; caller predInterSearch :2367).  For each of the n (PU, list, refIdx) rows and each of its
 * numAmvpCand candidates (amvpCand, already filled -- bFilled): clipMv, uni-directional luma prediction at the candidate (xPredInterBlk, rounded
 * and clipped), SAD against the original block + getCost( mvpIdxBits[i] ); the FIRST candidate with the smallest cost wins (`uiBestCost >
 * uiTmpCost`).  In place: mvPredHor / mvPredVer (the unclipped candidate), mvpIdx; with addIdxBits the winner's index bits are added to `bits`
 * as predInterSearch does right after the call (:2381).  d_distBiP (may be NULL): the winning template cost per row (*puiDistBiP).
 * uniformSize != 0: every row is maxWidth x maxHeight (uniform SAD kernel). */
int vtmhip_xEstimateMvPredAMVP_batch_dev( vtmhip_ctx *ctx, const vtmhip_pic_params *pic, const int16_t *d_orgBase, const int16_t *d_refBase,
                                          vtmhip_me_job *d_jobs, int n, int maxWidth, int maxHeight, int uniformSize, int addIdxBits, uint64_t *d_distBiP );

/* ---- motion compensation / bi-pred buffer ops ------------------------------------------------------------------------ */
typedef struct
{
  int64_t refOff, dstOff;       /* refOff: block position with MV (0,0) in the reference plane */
  int32_t refStride, dstStride;
  int16_t width, height;
  int32_t mvHor, mvVer;         /* internal 1/16 precision */
  uint8_t bi;                   /* 0: rounded + clipped samples (uni-pred); 1: 14-bit intermediates for addAvg */
  uint8_t bitDepth, useAltHpelIf;
  uint8_t chroma;               /* 0: luma plane, 8-tap, width/height/offsets in luma samples; 1: a 4:2:0 chroma plane, 4-tap at 1/32 phase --
                                   width/height/refOff/dstOff in samples of THAT plane, the vector still in luma 1/16 units */
} vtmhip_mc_job;

/* InterPrediction::xPredInterBlk without BDOF/DMVR/RPR/wrap-around (InterPrediction.cpp:660-815), luma and 4:2:0 chroma blocks mixed
 * freely in one batch (vtmhip_mc_job::chroma); maxWidth/maxHeight bound the block sizes of the batch (2..128). */
int vtmhip_mc_batch_dev( vtmhip_ctx *ctx, const int16_t *d_refBase, int16_t *d_dstBase, const vtmhip_mc_job *d_jobs, int n, int maxWidth,
                         int maxHeight );
/* the same call under its first name (luma-only callers) */
int vtmhip_mc_luma_batch_dev( vtmhip_ctx *ctx, const int16_t *d_refBase, int16_t *d_dstBase, const vtmhip_mc_job *d_jobs, int n, int maxWidth,
                              int maxHeight );

/* InterPrediction::motionCompensation for one PU and one plane (InterPrediction.cpp:445-660: xPredInterUni, or xPredInterBi with the
 * default-weight xWeightedAverage = PelBuf::addAvg :1354-1435), with the consumer of the prediction optionally fused in. */
typedef struct
{
  int64_t orgOff;               /* block in the original plane (epilogue 1 / 2) */
  int64_t refOff[2];            /* block position with MV (0,0) in the list-0 / list-1 reference plane (both inside d_refBase) */
  int64_t predOff, outOff;      /* prediction block inside d_predBase, epilogue output inside d_outBase */
  int32_t orgStride, refStride[2], predStride, outStride;
  int32_t mv[2][2];             /* [list][hor, ver], internal 1/16 luma precision */
  int16_t width, height;
  uint8_t mode;                 /* 0: uni-prediction from list 0, 1: from list 1, 2: bi-prediction (two 14-bit predictions, addAvg) */
  uint8_t epilogue;             /* 0: none; 1: out = org - pred (residual, InterSearch.cpp:7260-7262); 2: out = 2*org - pred (removeHighFreq) */
  uint8_t bitDepth, useAltHpelIf, chroma;
  uint8_t route;                /* 0: every call processes the job; a driver that launches BOTH vtmhip_motion_compensation_batch_dev and vtmhip_bdof_batch_dev over
                                   one table marks each job on the device: 1 = BDOF's (the plain call skips it), 2 = the plain call's (BDOF skips it) */
  int16_t bcwWeight;            /* epilogue 2 only: 0 or 4 = out = 2*org - pred; another getBcwWeight( cu.BcwIdx, searched list ) in {-2, 3, 5, 10}: out = removeWeightHighFreq
                                   = ( org * w0 - pred * w1 + 2^15 ) >> 16 with normalizer = ( 2^16 + |w| / 2 ) / w, w0 = normalizer * 8, w1 = ( 8 - w ) * normalizer (Buffer.h:417-460) */
} vtmhip_pred_job;

/* d_predBase and d_outBase may each be NULL (that output is skipped); d_orgBase is needed when d_outBase is given. */
int vtmhip_motion_compensation_batch_dev( vtmhip_ctx *ctx, const int16_t *d_orgBase, const int16_t *d_refBase, int16_t *d_predBase, int16_t *d_outBase,
                                          const vtmhip_pred_job *d_jobs, int n, int maxWidth, int maxHeight );

/* lanes a block gets in vtmhip_motion_compensation_batch_dev and in the template-cost pass of vtmhip_xEstimateMvPredAMVP_batch_dev under the hint maxWidth x maxHeight:
 * 8 (up to 64 samples: eight blocks per wave), 16 (up to 256: four per wave), 64 (up to 1024: a wave per block) or 256 (the workgroup per block); 0 when a side is
 * outside 2 .. 128.  Host arithmetic, no device needed. */
int vtmhip_mc_lanes_per_block( int maxWidth, int maxHeight );

typedef struct
{
  int64_t aOff, bOff, dstOff;
  int32_t aStride, bStride, dstStride;
  int16_t width, height;
  uint8_t bitDepth;
  int8_t  bcwWeight;            /* the BCW calls only: g_BcwWeights[bcwIdx] in {-2, 3, 4, 5, 10} (of 8), see there */
  uint8_t pad1, pad2;
  int32_t pad3;
} vtmhip_pelop_job;

/* PelBuf::removeHighFreq (Buffer.cpp:475-520; bi-pred ME target, InterSearch.cpp:3320-3326): dst = 2*org - pred, unclipped */
int vtmhip_remove_high_freq_batch_dev( vtmhip_ctx *ctx, const int16_t *d_orgBase, const int16_t *d_predBase, int16_t *d_dstBase,
                                       const vtmhip_pelop_job *d_jobs, int n );
/* PelBuf::subtract (residual = org - pred; CodingStructure resi buffer, InterSearch.cpp:7260-7262) */
int vtmhip_subtract_batch_dev( vtmhip_ctx *ctx, const int16_t *d_aBase, const int16_t *d_bBase, int16_t *d_dstBase, const vtmhip_pelop_job *d_jobs, int n );
/* PelBuf::addAvg (Buffer.cpp:467-507): dst = clip((src0 + src1 + offset) >> shift) on 14-bit intermediates */
int vtmhip_add_avg_batch_dev( vtmhip_ctx *ctx, const int16_t *d_src0Base, const int16_t *d_src1Base, int16_t *d_dstBase,
                              const vtmhip_pelop_job *d_jobs, int n );

/* BCW (Buffer.h:417-460, Buffer.cpp:365-397).  removeWeightHighFreq: the bi-pred ME target when the searched list carries weight job.bcwWeight,
 * dst = ( org * (n << 3) - pred * ((8 - w) * n) + 2^15 ) >> 16 with n = (2^16 + |w >> 1|) / w, unclipped (g_pelBufOP.removeWeightHighFreq4/8).
 * addWeightedAvg: dst = clip( ( src0 * (8 - w) + src1 * w + offset ) >> shift ), job.bcwWeight = w = the LIST-1 weight g_BcwWeights[bcwIdx]. */
int vtmhip_remove_weight_high_freq_batch_dev( vtmhip_ctx *ctx, const int16_t *d_orgBase, const int16_t *d_predBase, int16_t *d_dstBase,
                                              const vtmhip_pelop_job *d_jobs, int n );
int vtmhip_add_weighted_avg_batch_dev( vtmhip_ctx *ctx, const int16_t *d_src0Base, const int16_t *d_src1Base, int16_t *d_dstBase,
                                       const vtmhip_pelop_job *d_jobs, int n );

/* BDOF: InterPrediction::xPredInterBi with bioApplied for bi-predicted LUMA PUs (InterPrediction.cpp:527-660: xSubPuBio :352-443 cuts the PU into
 * regions of at most 16 x 16, xPredInterBlk(..., bioApplied) :733-810 predicts each from both lists inside a ring of integer samples, and
 * xWeightedAverage -> applyBiOptFlow :1233-1334 refines every 4 x 4 unit with g_pelBufOP.bioGradFilter / calcBIOSums / addBIOAvg4, Buffer.cpp:88-200).
 * The job table is the one of vtmhip_motion_compensation_batch_dev: the caller sends here the PUs for which the reference sets bioApplied (:527-572:
 * true bi-prediction with equal and opposite POC distances, w, h >= 8, w*h >= 128, no affine / SMVD / CIIP / BCW / weighted prediction); mode must be
 * 2, chroma 0 (the chroma planes of such a PU take the plain addAvg path).  The epilogue and the NULL rules are those of that call. */
int vtmhip_bdof_batch_dev( vtmhip_ctx *ctx, const int16_t *d_orgBase, const int16_t *d_refBase, int16_t *d_predBase, int16_t *d_outBase,
                           const vtmhip_pred_job *d_jobs, int n, int maxWidth, int maxHeight );

/* DMVR: InterPrediction::xProcessDMVR (InterPrediction.cpp:1997-2195) for the LUMA plane of the bi-predicted PUs for which the reference's
 * PU::checkDMVRCondition holds (merge mode, equal and opposite POC distances, w, h >= 8, w*h >= 128, default weights ...; xPredInterBi :576-583).
 * Per sub-PU of at most 16 x 16: xPrefetch, bilinear xinitMC, the 25-point mirrored integer refinement (xDMVRCost / xBIPMVRefine :1819-1927), the
 * parametric error surface (:1733-1817, 1929-1947), xPad + xFinalPaddedMCForDMVR (:1709-1731, 1845-1917) and xWeightedAverage, with BDOF
 * (vtmhip_bdof_batch_dev's arithmetic) where bioApplied is set and the sub-PU's matching cost is not below 2*dx*dy (:2139). */
typedef struct
{
  int64_t orgOff;               /* block in the original plane (epilogue 1 / 2) */
  int64_t refOff[2];            /* PU position with MV (0,0) in the list-0 / list-1 reference plane (both inside d_refBase) */
  int64_t predOff, outOff;      /* prediction block inside d_predBase, epilogue output inside d_outBase */
  int32_t orgStride, refStride[2], predStride, outStride;
  int32_t mv[2][2];             /* the merge vectors, [list][hor, ver], internal 1/16 precision */
  int32_t puX, puY;             /* luma position of the PU in the picture: clipMv (Mv.cpp:56-74) */
  int16_t width, height;
  uint8_t bioApplied;           /* what xPredInterBi decided for the PU (:527-572) */
  uint8_t epilogue;             /* as vtmhip_pred_job */
  uint8_t bitDepth, pad0;
  int32_t mvdRow;               /* chroma call only: the d_mvd row (= job index of the luma call) that holds this PU's vector differences */
} vtmhip_dmvr_job;
/* pic: picW / picH / ctuSize / bitDepth.  d_mvd (may be NULL): pu.mvdL0SubPu, int32 [n][regions][2] with regions = ceil(maxWidth/16) * ceil(maxHeight/16),
 * sub-PUs in the reference's raster order. */
int vtmhip_dmvr_batch_dev( vtmhip_ctx *ctx, const vtmhip_pic_params *pic, const int16_t *d_orgBase, const int16_t *d_refBase, int16_t *d_predBase,
                           int16_t *d_outBase, const vtmhip_dmvr_job *d_jobs, int n, int maxWidth, int maxHeight, int32_t *d_mvd );

/* One 4:2:0 chroma plane of the same PUs, after the luma call: a sub-PU whose difference is zero is predicted from the reference pictures, a moved one
 * out of its (w/2+3) x (h/2+3) window -- prefetched with the MERGE vector (xPrefetch forLuma = 0, :1666-1708), replicated by one sample (xPad: padsize =
 * 2 >> scaleY, :1709-1731), addressed with the whole-sample part of the refined vector (xFinalPaddedMCForDMVR :1879-1905) -- then the plain addAvg.
 * The jobs keep width / height / puX / puY / mv in LUMA units; refOff / strides / orgOff / predOff / outOff address THAT chroma plane (refOff: the PU's
 * position in it); d_mvd, maxWidth and maxHeight are those of the luma call (same `regions`), vtmhip_dmvr_job::mvdRow picks the row. */
int vtmhip_dmvr_chroma_batch_dev( vtmhip_ctx *ctx, const vtmhip_pic_params *pic, const int16_t *d_orgBase, const int16_t *d_refBase, int16_t *d_predBase,
                                  int16_t *d_outBase, const vtmhip_dmvr_job *d_jobs, int n, int maxWidth, int maxHeight, const int32_t *d_mvd );

/* InterpolationFilter::m_weightedGeoBlk (InterpolationFilter.h:99; xWeightedGeoBlk InterpolationFilter.cpp:902-957, x86/InterpolationFilterX86.h:1343-1470;
 * callers InterPrediction::weightedGeoBlk InterPrediction.cpp:1642-1661, EncCu.cpp:3004,3030): blend of the two GEO partitions' 14-bit predictions,
 *   dst = clip( ( w * src0 + (8 - w) * src1 + offset ) >> shift ),  shift = max(2, 14 - bitDepth) + 3,  offset = (1 << (shift-1)) + (8192 << 3),
 * with w = weight[y * weightStride + x * stepX] in 0..8.  The caller (the trampoline that receives pu / splitDir) derives weight, stepX and
 * weightStride from g_GeoParams / g_angle2mirror / g_weightOffset exactly as the reference does: stepX = +-1 (luma) or +-2 (4:2:0 chroma),
 * weightStride = +-GEO_WEIGHT_MASK_SIZE << scaleY (the scalar version's `width * stepX + stepY`). */
int vtmhip_weightedGeoBlk( vtmhip_ctx *ctx, const int16_t *src0, int src0Stride, const int16_t *src1, int src1Stride, int16_t *dst, int dstStride, int width,
                           int height, const int16_t *weight, int stepX, int weightStride, int bitDepth, int clipMin, int clipMax );
typedef struct
{
  int64_t src0Off, src1Off, dstOff;   /* samples inside d_srcBase / d_srcBase / d_dstBase */
  int64_t weightOff;                  /* first weight (top-left output sample) inside d_weightBase */
  int32_t src0Stride, src1Stride, dstStride, weightStride;
  int16_t width, height, stepX, pad;
} vtmhip_geo_blend_job;
/* n GEO blends in one launch (e.g. every tested (split, candidate pair) of a CU, EncCu.cpp:2990-3035); d_weightBase: the g_globalGeoWeights planes,
 * uploaded once */
int vtmhip_weightedGeoBlk_batch_dev( vtmhip_ctx *ctx, const int16_t *d_srcBase, int16_t *d_dstBase, const int16_t *d_weightBase,
                                     const vtmhip_geo_blend_job *d_jobs, int n, int bitDepth, int clipMin, int clipMax );

/* ---- interpolation ----------------------------------------------------------------------------------------------- */
typedef struct
{
  int64_t srcOff, dstOff;   /* samples; srcOff addresses the output-aligned sample */
  int32_t srcStride, dstStride;
  int16_t width, height;
  uint8_t vertical, taps /* 8, 4, 2; 0 = filterCopy */, isFirst, isLast;
  int16_t coeff[8];
  int16_t clipMin, clipMax;
  uint8_t bitDepth, biMCForDMVR, pad0, pad1;
} vtmhip_if_job;

/* n filter / copy passes, one workgroup each (hook B6 plane generation, motion compensation) */
int vtmhip_if_batch_dev( vtmhip_ctx *ctx, const int16_t *d_srcBase, int16_t *d_dstBase, const vtmhip_if_job *d_jobs, int n );

/* ---- fractional motion search: one InterSearch::xPatternSearchFracDIF per job (hook B6) ------------------------------ */
typedef struct
{
  int64_t orgOff, refOff;   /* as vtmhip_tz_job: PU top-left in the original plane / same position (MV 0,0) in the reference plane */
  int32_t orgStride, refStride;
  int16_t width, height;    /* not 4x4 (no 4x4 inter PU exists; the reference switches tap tables there, InterpolationFilter.cpp:786-789) */
  int16_t intX, intY;       /* rcMvInt: result of the integer search */
  int32_t predHor, predVer; /* RdCost::setPredictor, quarter-sample units */
  double  motionLambda;
  uint8_t useHad;           /* HadamardME && !DisableSATDForRD: SATD, else SAD.  For bitDepth <= 10 the tiled kernel forms the SATD differences in 16 bits (as the
                               reference's SIMD does): the original samples must lie in [-3072, 3071] -- picture samples or the bi-pred target 2*org - pred */
  uint8_t useAltHpelIf;     /* cu.imv == IMV_HPEL */
  uint8_t imvShift;         /* 0: half + quarter refinement; 1 (IMV_HPEL): half only */
  uint8_t bitDepth;
  int32_t wideOrg;          /* != 0: the original samples may leave [-3072, 3071] (a BCW-weighted bi-pred target: up to +-5115): the tiled kernel takes its 32-bit SATD path */
} vtmhip_frac_job;

typedef struct
{
  int16_t  halfX, halfY;   /* rcMvHalf in {-1,0,1}^2 */
  int16_t  qterX, qterY;   /* rcMvQter in {-1,0,1}^2; final MV (quarter units) = (int << 2) + (half << 1) + qter */
  uint64_t cost;           /* ruiCost */
} vtmhip_frac_result;

/* maxWidth/maxHeight: upper bounds of the job sizes in this batch (they size the per-workgroup LDS window).
 * uniformSquare != 0: the caller guarantees that EVERY job is exactly maxWidth x maxHeight -- a square in {8,16,32,64,128} or one of the split
 * shapes 16x8, 32x8, 32x16, 64x16, 64x32 in either orientation (their SATD tiles are the reference's 16x8 / 8x16 Hadamards) -- and that all
 * jobs share imvShift; the library then uses the tiled kernel (one lane per (PU, candidate, 8x8 tile)); other uniform shapes and
 * 0 = any mix of sizes: one wave per PU. */
int vtmhip_frac_search_batch_dev( vtmhip_ctx *ctx, const int16_t *d_orgBase, const int16_t *d_refBase, const vtmhip_frac_job *d_jobs, int n,
                                  int maxWidth, int maxHeight, int uniformSquare, vtmhip_frac_result *d_results );

/* ---- transform / quantisation: one TU per job --------------------------------------------------------------------- */
typedef struct
{
  int64_t srcOff, dstOff;   /* xT: residual samples -> coefficients; xIT: coefficients -> residual samples (offsets in elements) */
  int32_t srcStride;        /* xT: residual stride (CS resi stride); coefficients are always W x H contiguous */
  int32_t dstStride;        /* xIT: residual stride */
  int16_t width, height;    /* 1..64 (MAX_TB_SIZEY) */
  uint8_t typeHor, typeVer; /* VTMHIP_DCT2 / DCT8 / DST7 as TrQuant::getTrTypes chose them */
  uint8_t bitDepth, pad;    /* bitDepth: 8..12, the library's sample contract (not checked per job); xT takes residuals within +-(2^bitDepth - 1) */
} vtmhip_tr_job;

/* TrQuant::xT (TrQuant.cpp:776-851) for n TUs.  d_sumAbs (may be NULL): sum |coef| per TU (MTS pre-selection, :986-990). */
int vtmhip_xT_batch_dev( vtmhip_ctx *ctx, const int16_t *d_resiBase, int32_t *d_coefBase, const vtmhip_tr_job *d_jobs, int n, int maxWidth,
                         int maxHeight, int32_t *d_sumAbs );
/* TrQuant::xIT (TrQuant.cpp:853-923) */
int vtmhip_xIT_batch_dev( vtmhip_ctx *ctx, const int32_t *d_coefBase, int16_t *d_resiBase, const vtmhip_tr_job *d_jobs, int n, int maxWidth,
                          int maxHeight );

typedef struct
{
  int64_t srcOff, dstOff;   /* W x H contiguous TCoeff blocks */
  int16_t width, height;
  int16_t qpPer, qpRem;     /* QpParam::per / rem (Quant.cpp:65-104): base QP = QP + 6 * (bitDepth - 8), 0 .. 63 + 6 * (bitDepth - 8); for transform skip the
                               caller applies QpParam's floor of 4 on the base QP */
  uint8_t bitDepth, isIRAP, isTransformSkip, pad;   /* bitDepth: 8..12, the library's sample contract (not checked per job) */
  int32_t pad2;
} vtmhip_quant_job;

/* Quant::quant, flat scaling list, no sign-bit hiding (Quant.cpp:955-1038): levels, optional deltaU, absSum per TU */
int vtmhip_quant_batch_dev( vtmhip_ctx *ctx, const int32_t *d_coefBase, int32_t *d_qBase, int32_t *d_deltaUBase, const vtmhip_quant_job *d_jobs, int n,
                            int32_t *d_absSum );
/* Quant::dequant, flat scaling list (Quant.cpp:357-482) */
int vtmhip_dequant_batch_dev( vtmhip_ctx *ctx, const int32_t *d_qBase, int32_t *d_coefBase, const vtmhip_quant_job *d_jobs, int n );

/* ---- fused residual-coding chain: hooks B8 + B9 in one launch -------------------------------------------------------------
 * per TU and transform candidate: TrQuant::xT -> Quant::quant -> Quant::dequant -> TrQuant::xIT -> SSE(residual, reconstruction)
 * (xEstimateInterResidualQT, InterSearch.cpp:6637-6733, minus the CABAC bit estimate between quant and dequant).  2-D TUs only. */
typedef struct
{
  int64_t resiOff;          /* residual samples (int16) */
  int64_t outOff;           /* W x H contiguous block inside d_levelsBase / d_recBase (when those are given) */
  int32_t resiStride;
  int16_t width, height;    /* 2..64 */
  int16_t qpPer, qpRem;     /* as vtmhip_quant_job */
  uint8_t typeHor, typeVer, bitDepth, isIRAP;   /* bitDepth: 8..12, the library's sample contract (not checked per job); residuals within +-(2^bitDepth - 1) */
  int32_t pad;
  int32_t chromaAdj;        /* bytes 36 .. 39, the struct's tail padding until now: vtmhip_tu_chain_crs_batch_dev reads tu.getChromaAdj() here, or 0 for no scaling (the
                               LMCS section below); every other entry ignores them */
} vtmhip_tu_job;

typedef struct
{
  uint64_t sse;             /* getDistPart( DF_SSE ) of residual vs reconstructed residual */
  int32_t  sumAbs;          /* sum |coef| after xT (MTS pre-selection cost, TrQuant.cpp:986-990) */
  int32_t  absSum;          /* uiAbsSum of Quant::quant (cbf = absSum > 0) */
} vtmhip_tu_result;

/* d_levelsBase (quantised levels for the host's CABAC estimate) and d_recBase (reconstructed residual) may be NULL.
 * uniformSize != 0: the caller guarantees every TU is exactly maxWidth x maxHeight with a real transform (no VTMHIP_TRSKIP) -> register-blocked kernel
 * (both sides >= 8) or one lane per TU (4x4, 8x4, 4x8); other uniform shapes (16x4 ...) take the generic kernel. */
int vtmhip_tu_chain_batch_dev( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_tu_job *d_jobs, int n, int maxWidth, int maxHeight,
                               int uniformSize, int32_t *d_levelsBase, int16_t *d_recBase, vtmhip_tu_result *d_results );

/* The transform-skip candidate (tu.mtsIdx == MTS_SKIP; TrQuant.cpp:976-980 xTransformSkip, :925-941 xITransformSkip; Quant.cpp:966-997 with
 * useTransformSkip) of the same chain for a uniform batch: every job width x height (powers of two, 4..32) with typeHor == VTMHIP_TRSKIP and
 * qpPer / qpRem = QpParam::per( true ) / rem( true ).  results[i].sumAbs = sum |residual| (unscaled: vtmhip_mts_select2 applies scaleSAD).
 * vtmhip_tu_chain_batch_dev with uniformSize == 0 takes VTMHIP_TRSKIP jobs mixed with the others. */
int vtmhip_tu_ts_chain_batch_dev( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_tu_job *d_jobs, int n, int width, int height,
                                  int32_t *d_levelsBase, int16_t *d_recBase, vtmhip_tu_result *d_results );

/* The MTS pre-selection of a whole level on the device (vtmhip_mts_select2 per TU): d_results holds numCand runs of numTU results one after the other (the
 * layout vtmhip_pis_level_run uses: results[c * numTU + t]), mtsIdx[c] = the candidate's tu.mtsIdx (1 = transform skip: sumAbs is sum |residual|);
 * d_test[c * numTU + t] = 1 when candidate c of TU t survives.  numCand <= 8. */
int vtmhip_mts_select_batch_dev( vtmhip_ctx *ctx, const vtmhip_tu_result *d_results, int numTU, int numCand, const uint8_t *mtsIdx, int width, int height,
                                 int bitDepth, int maxLog2TrDynamicRange, int maxCand, uint8_t *d_test );

/* TrQuant::xT only, for a batch the caller promises to be uniform (every TU width x height, powers of two 8..64) -- the forward transforms of all
 * MTS candidates of TrQuant::transformNxN( ..., trModes, maxCand ) (TrQuant.cpp:950-1019): same job table as the fused chain (qp fields unused);
 * coefficients (H x W contiguous) go to d_coefBase + outOff, results[i].sumAbs = sum |coef| for vtmhip_mts_select(). */
int vtmhip_xT_uniform_batch_dev( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_tu_job *d_jobs, int n, int width, int height, int32_t *d_coefBase,
                                 vtmhip_tu_result *d_results );

/* ---- joint Cb-Cr residual coding (JCCR / ICT): TrQuant::m_fwdICT[-3..3] / m_invICT[-3..3] and the joint chroma candidate ---------------
 * (CommonLib/TrQuant.cpp:86-157 fwdTransformCbCr / invTransformCbCr, :619-687 fwdTransformICT / invTransformICT / selectICTCandidates;
 * g_ictModes Rom.cpp:527; TU::getICTMode UnitTools.cpp:3825; callers InterSearch.cpp:6813-7032 and IntraSearch::xRecurIntraChromaCodingQT.)
 *   mode = g_ictModes[signFlag][cbfMask] = { { 0, 3, 1, 2 }, { 0, -3, -1, -2 } };  s = mode < 0 ? -1 : 1;  `/` truncates toward zero, Pel() wraps to
 *   int16, `>>` is arithmetic:
 *     +-1: c = Pel( (4 cb + s 2 cr) / 5 )                      d1 += (cb - c)^2 + (cr - ((s c) >> 1))^2      inverse: cr = (s cb) >> 1
 *     +-2: c = Pel( (cb + s cr) / 2 )                          d1 += (cb - c)^2 + (cr - s c)^2               inverse: cr = cb;  -2: cr = cb == -32768 ? 32767 : -cb
 *     +-3: c = Pel( (4 cr + s 2 cb) / 5 ), stored in the Cr block  d1 += (cb - ((s c) >> 1))^2 + (cr - c)^2  inverse: cb = (s cr) >> 1
 *       0: no joint residual; d1 = sum cb^2, d2 = sum cr^2
 *   The coded component is Cb for cbfMask 2 and 3 and Cr for cbfMask 1.  Sums are int64.
 * Sample range: the entries take ANY int16 residual (the Pel wrap is part of the rule).  Encoder residuals lie within +-(2^bitDepth - 1), which makes a joint
 * residual of modes +-1 / +-3 reach 6 (2^bitDepth - 1) / 5 (1227 at 10 bits, 4914 at 12) -- outside the +-(2^bitDepth - 1) vtmhip_tu_job documents for xT.  The
 * joint chain holds for it on all three launch paths, and for every int16 joint residual: the generic and the one-lane kernels accumulate in 32 bits as the
 * reference does; the register-blocked kernel's packed first pass multiplies int16 pairs into a 32-bit accumulator (|sum| <= 64 * 32768 * 90 < 2^31) and its
 * output stays below sum|m| * 32768 >> (log2 N + bitDepth - 9) <= 2^22, inside the 24-bit multiplies of the second pass.
 * Out of scope: ACT, the picture-level sign decision
 * (EncSlice::setJointCbCrModes: the caller passes signFlag), the CABAC estimate, the level-order picture driver, a host C++ mirror. */

/* (*m_fwdICT[mode])( resCb, resCr, resC1, resC2 ) on host pointers, staged like vtmhip_xGetSAD; mode -3 .. 3, width / height 1 .. 64.  The joint residual goes
 * to c1 (modes +-1, +-2) or c2 (modes +-3); the other block -- both for mode 0 -- is not written and may be NULL.  dist = { d1, d2 }. */
int vtmhip_fwdTransformCbCr( vtmhip_ctx *ctx, int mode, const int16_t *cb, int cbStride, const int16_t *cr, int crStride, int16_t *c1, int c1Stride,
                             int16_t *c2, int c2Stride, int width, int height, int64_t dist[2] );
/* (*m_invICT[mode])( resCb, resCr ), in place on host pointers */
int vtmhip_invTransformCbCr( vtmhip_ctx *ctx, int mode, int16_t *cb, int cbStride, int16_t *cr, int crStride, int width, int height );

typedef struct
{
  int64_t cbOff, crOff;         /* the Cb / Cr residual blocks inside d_resiBase */
  int64_t outOff;               /* the joint residual of cbfMask m (W x H contiguous) goes to d_jointBase + outOff + (m - 1) * W * H */
  int32_t cbStride, crStride;
  int16_t width, height;        /* 1 .. 64 */
  uint8_t signFlag;             /* picHeader.getJointCbCrSignFlag() */
  uint8_t maskBits;             /* bit m (m = 1 .. 3) set: write the joint residual of cbfMask m */
  uint8_t pad0, pad1;
} vtmhip_ict_job;

/* TrQuant::fwdTransformICT for cbfMask 0 .. 3 of n (Cb, Cr) pairs -- the loop of selectICTCandidates (:648-658): d_dist[i][m] = { d1, d2 } of cbfMask m
 * (int64 [n][4][2]) and the requested joint residual planes.  d_jointBase may be NULL when no job asks for a plane. */
int vtmhip_ict_fwd_batch_dev( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_ict_job *d_jobs, int n, int16_t *d_jointBase, int64_t *d_dist );

/* TrQuant::selectICTCandidates' decision from the four distance pairs (host arithmetic, no device): an inter CU tests { 3 }; an intra CU the best cbfMask whose
 * d1 beats min( d1[0], d2[0] ) and the runner-up within 9 / 8 of it (3 / 2 when no mask won), integer arithmetic as :660-686.  masks: the cbfMasks to test in
 * the reference's order, *numMasks of them (0 .. 2). */
int vtmhip_ict_select( const int64_t dist[4][2], int isIntra, int masks[2], int *numMasks );

typedef struct
{
  int64_t cbOff, crOff;     /* the ORIGINAL Cb / Cr residual blocks inside d_resiBase (one stride: both come from the same residual buffer) */
  int64_t outOff;           /* W x H contiguous block inside d_levelsBase / d_recCbBase / d_recCrBase (where those are given) */
  int32_t resiStride;
  int16_t width, height;    /* 2..64 */
  int16_t qpPer, qpRem;     /* QpParam( tu, codeCompId ).per / rem (Quant.cpp:112-125: the JOINT_CbCr offsets and table when |mode| == 2); the device does not derive it */
  uint8_t typeHor;          /* VTMHIP_DCT2 (DCT2 / DCT2) or VTMHIP_TRSKIP (both sides <= 32; qpPer / qpRem = per( true ) / rem( true )) */
  uint8_t bitDepth;         /* 8..12 */
  uint8_t isIRAP;
  uint8_t cbfMask;          /* tu.jointCbCr: 1 .. 3 */
  uint8_t signFlag;         /* picHeader.getJointCbCrSignFlag() */
#pragma pack( push, 1 )     /* the overlay starts at the odd byte 41: byte-packed, chromaAdj still sits at the even byte 42 */
  union
  {
    uint8_t pad[7];         /* every entry but vtmhip_jccr_chain_crs_batch_dev ignores these seven bytes */
    struct
    {
      uint8_t  reserved0;
      uint16_t chromaAdj;   /* vtmhip_jccr_chain_crs_batch_dev: tu.getChromaAdj(), or 0 for no scaling (the LMCS section below) */
      uint8_t  reserved1[4];
    };
  };
#pragma pack( pop )
} vtmhip_jccr_job;

typedef struct
{
  uint64_t sseCb, sseCr;    /* getDistPart( DF_SSE ) of the ORIGINAL Cb / Cr residual against the block the inverse ICT rebuilt (InterSearch.cpp:6910-6998) */
  int64_t  fwdDist;         /* d1 of the job's mode (the forward ICT's own distance) */
  int32_t  sumAbs;          /* sum |coef| of the joint residual after xT (transform skip: sum |joint residual|) */
  int32_t  absSum;          /* uiAbsSum of Quant::quant on the coded component */
} vtmhip_jccr_result;

/* The joint chroma candidate of xEstimateInterResidualQT, one launch, nothing through global memory in between: per job load Cb and Cr once, forward ICT of the
 * job's mode, xT -> Quant::quant -> Quant::dequant -> xIT (or the transform-skip copies) on the joint residual with the arithmetic of vtmhip_tu_chain_batch_dev,
 * inverse ICT, both SSEs.  Zero levels need no special case (they reconstruct zero and the inverse ICT of zero is zero).  d_levelsBase (levels of the coded
 * component), d_recCbBase and d_recCrBase may be NULL.  uniformSize as in vtmhip_tu_chain_batch_dev: every job exactly maxWidth x maxHeight with VTMHIP_DCT2 ->
 * one lane per pair (4x4, 8x4, 4x8) or the register-blocked kernel (power-of-two sides >= 8); 0: any mix, sides 2..64, on the generic LDS kernel.
 * The job table is read back (n * 48 bytes, one stream synchronisation) and checked on the host before anything is launched: a cbfMask outside 1 .. 3, a
 * typeHor other than the two above, transform skip on a side > 32, a size outside 2 .. maxWidth / maxHeight or (uniformSize) a job of another shape or with
 * transform skip return VTMHIP_E_INVALID and launch nothing.  n == 0 is VTMHIP_OK. */
int vtmhip_jccr_chain_batch_dev( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_jccr_job *d_jobs, int n, int maxWidth, int maxHeight, int uniformSize,
                                 int32_t *d_levelsBase, int16_t *d_recCbBase, int16_t *d_recCrBase, vtmhip_jccr_result *d_results );

int vtmhip_jccr_struct_size( int which );   /* sizeof() of 0 vtmhip_ict_job, 1 vtmhip_jccr_job, 2 vtmhip_jccr_result; -1 otherwise (vtmhip_struct_size keeps its list) */

/* ---- LMCS (luma mapping with chroma scaling), the residual path -----------------------------------------------------------------------------
 * The steps of the reference an encode with LMCSEnable takes around the residual of an inter CU:
 *   luma residual in the mapped domain     resi = fwdLUT[org] - fwdLUT[pred]              InterSearch.cpp:7285-7296 (encodeResAndCalcRdInterCU)
 *   chroma residual scaling (CRS) of a TU  scaleSignal( adj, 1 ) before transformNxN, scaleSignal( adj, 0 ) after invTransformNxN, DF_SSE against the
 *                                          UNSCALED residual                             InterSearch.cpp:6628-6632, 6728-6733; Buffer.cpp:415-464
 *   the same around the joint candidate    scale Cb and Cr, forward ICT, chain, inverse ICT, inverse-scale both, DF_SSE against the unscaled residuals
 *                                                                                        InterSearch.cpp:6822-6823, 6838-6842, 6977-6998
 *   reconstruction                         reco = clip( fwdLUT[pred] + resi )             InterSearch.cpp:7540-7551
 *   final distortion                       DF_SSE_WTD with the inverse reshape of cur     InterSearch.cpp:7585-7596 (vtmhip_sse_wtd_batch_dev above)
 * The two sample rules of AreaBuf<Pel>::scaleSignal (Buffer.cpp:415-464), CSCALE_FP_PREC = 11, M = (1 << bitDepth) - 1, `/` truncates toward zero, sgn(0) = +1:
 *   forward (dir 1):  a = |v|;  out = Pel( Clip3( -M, M, sgn(v) * ( ((a << 11) + (scale >> 1)) / scale ) ) )
 *   inverse (dir 0):  c = Clip3( -M-1, M, v );  a = |c|;  out = Clip3( -32768, 32767, sgn(c) * ( (a * scale + 1024) >> 11 ) )
 * Scale contract: 1 <= scale <= 32767 (VVC confines ChromaScaleCoeff to 256 .. 16384; Reshape.cpp:260-265 gives 2048 for empty bins); bitDepth 8 .. 12; any
 * int16 sample.  The division is exact (vtm_amd/csrc/lmcs.hpp has the argument).  A scale of 2048 is NOT a no-op on the inverse side: the input clip applies.
 * The adj of a TU comes from Reshape::calculateChromaAdjVpduNei on the host, which also keeps the lambda adjustment lambda / cRescale^2 (:6612-6613, 6917-6918).
 * Out of scope: the level-order picture driver, the host C++ mirror, an ICT-distance entry with a built-in scale, calculateChromaAdjVpduNei, ACT, the CABAC estimate. */

/* The chains with CRS fused in: same arguments, launch paths (bucketed, one lane per TU, register-blocked, generic) and argument checks as
 * vtmhip_tu_chain_batch_dev / vtmhip_jccr_chain_batch_dev; the per-job adj travels in the job (vtmhip_tu_job.chromaAdj, vtmhip_jccr_job.chromaAdj).
 *   adj == 0: the job runs unscaled.  Otherwise the kernel scales only when width * height > 4 -- the reference's own condition, so a caller may pass
 *   tu.getChromaAdj() unconditionally.
 *   plain chain: r -> the chain (or the transform-skip copies) on fwd(r) -> rec = inv(result); sse = SSE( r, rec ); d_recBase receives the inverse-scaled block;
 *     d_levelsBase, sumAbs and absSum are those of the SCALED residual.  The job table stays on the device, so an adj outside 0 .. 32767 counts as 0.
 *   joint chain: cb' = fwd(cb), cr' = fwd(cr); forward ICT of (cb', cr') -- fwdDist is the distance on the scaled pair; the chain; inverse ICT; inv() on both
 *     blocks; sseCb / sseCr against the original cb / cr.  The table is read back as before: an adj above 32767 returns VTMHIP_E_INVALID and launches nothing.
 * Transform-skip chroma jobs take these entries with uniformSize == 0 (vtmhip_tu_ts_chain_batch_dev has no CRS form). */
int vtmhip_tu_chain_crs_batch_dev( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_tu_job *d_jobs, int n, int maxWidth, int maxHeight,
                                   int uniformSize, int32_t *d_levelsBase, int16_t *d_recBase, vtmhip_tu_result *d_results );
int vtmhip_jccr_chain_crs_batch_dev( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_jccr_job *d_jobs, int n, int maxWidth, int maxHeight, int uniformSize,
                                     int32_t *d_levelsBase, int16_t *d_recCbBase, int16_t *d_recCrBase, vtmhip_jccr_result *d_results );

/* The reshaper's forward LUT (Reshape::getFwdLUT(), 1 << lumaBD entries, lumaBD 8 .. 12) for the two batched ops below.  Ordering and lifetime as
 * vtmhip_set_luma_level_weights (which holds the inverse LUT): ordered on the context's stream before every later launch, done when the call returns; call it
 * after every update of the reshaper.  vtmhip_lmcs_resi_batch_dev / vtmhip_lmcs_reco_batch_dev fail with VTMHIP_E_INVALID until it has been called. */
int vtmhip_set_lmcs_fwd_lut( vtmhip_ctx *ctx, const int16_t *fwdLut, int lumaBD );

/* AreaBuf<Pel>::rspSignal( lut ) (Buffer.cpp:399-413) in place on host pointers, staged like vtmhip_xGetSAD: buf[x] = lut[buf[x]].  width / height 1 .. 128,
 * lutSize 1 .. 65536; a sample outside [0, lutSize) returns VTMHIP_E_INVALID and leaves buf untouched. */
int vtmhip_rspSignal( vtmhip_ctx *ctx, int16_t *buf, int stride, int width, int height, const int16_t *lut, int lutSize );
/* AreaBuf<Pel>::scaleSignal( scale, dir, clpRng ) in place on host pointers: any int16 sample, scale 1 .. 32767, bitDepth 8 .. 12, width / height 1 .. 128.
 * dir != 0 with width == 1 returns VTMHIP_E_INVALID (the reference THROWs). */
int vtmhip_scaleSignal( vtmhip_ctx *ctx, int16_t *buf, int stride, int width, int height, int scale, int dir, int bitDepth );

typedef struct
{
  int64_t srcOff, dstOff;       /* samples inside d_srcBase / d_dstBase (the same buffer and offsets: in place) */
  int32_t srcStride, dstStride;
  int16_t width, height;        /* 1 .. 128 */
  uint16_t scale;               /* 1 .. 32767 */
  uint8_t dir;                  /* 1 forward, 0 inverse */
  uint8_t bitDepth;             /* 8 .. 12 */
} vtmhip_scale_job;

/* scaleSignal of n blocks, each with its own scale and direction, e.g. the scaled (Cb, Cr) pair selectICTCandidates of an intra CU needs before
 * vtmhip_ict_fwd_batch_dev.  The jobs are device-resident: a job outside the ranges above is skipped (its dst is not written). */
int vtmhip_scale_signal_batch_dev( vtmhip_ctx *ctx, const int16_t *d_srcBase, int16_t *d_dstBase, const vtmhip_scale_job *d_jobs, int n );

#define VTMHIP_LMCS_MAP_PRED 1   /* map the prediction through the forward LUT (clear for CIIP / IBC CUs, whose prediction is mapped already: InterSearch.cpp:7293) */
#define VTMHIP_LMCS_WRITE_MAPPED 2   /* resi op only: also write the mapped prediction to d_dstBase + dstOff */
typedef struct
{
  int64_t orgOff, predOff, resiOff, dstOff;   /* samples inside d_orgBase / d_predBase / d_resiBase / d_dstBase */
  int32_t orgStride, predStride, resiStride, dstStride;
  int16_t width, height;                      /* 1 .. 128 */
  uint8_t bitDepth;                           /* reco: the clip's bit depth, 8 .. 12 (resi: unused) */
  uint8_t flags;                              /* VTMHIP_LMCS_* */
  uint8_t pad0, pad1;
} vtmhip_lmcs_job;

/* resi = fwdLUT[org] - ( MAP_PRED ? fwdLUT[pred] : pred ) to d_resiBase + resiOff; with WRITE_MAPPED the (mapped) prediction goes to d_dstBase + dstOff
 * (d_dstBase may be NULL when no job asks).  Small blocks share a wave.  A LUT index is clamped into the table; a job with width / height outside 1 .. 128
 * or unknown flags is skipped. */
int vtmhip_lmcs_resi_batch_dev( vtmhip_ctx *ctx, const int16_t *d_orgBase, const int16_t *d_predBase, int16_t *d_resiBase, int16_t *d_dstBase,
                                const vtmhip_lmcs_job *d_jobs, int n );
/* reco = Clip3( 0, (1 << bitDepth) - 1, ( MAP_PRED ? fwdLUT[pred] : pred ) + resi ) to d_dstBase + dstOff (orgOff unused) */
int vtmhip_lmcs_reco_batch_dev( vtmhip_ctx *ctx, const int16_t *d_predBase, const int16_t *d_resiBase, int16_t *d_dstBase, const vtmhip_lmcs_job *d_jobs, int n );

int vtmhip_lmcs_struct_size( int which );   /* sizeof() of 0 vtmhip_lmcs_job, 1 vtmhip_scale_job; -1 otherwise (vtmhip_struct_size keeps its list) */

/* ---- affine ME gradients: AffineGradientSearch::m_HorizontalSobelFilter / m_VerticalSobelFilter / m_EqualCoeffComputer -----------
 * (AffineGradientSearch.h:50-54, AffineGradientSearch.cpp:62-170; caller xAffineMotionEstimation, InterSearch.cpp:5340-5775) */
typedef struct
{
  int64_t predOff;      /* prediction block (int16) */
  int64_t resiOff;      /* error block org - pred (int16) */
  int64_t derivHOff;    /* horizontal derivative plane (int32) inside d_derivBase */
  int64_t derivVOff;    /* vertical derivative plane */
  int32_t predStride, resiStride, derivStride;
  int16_t width, height;   /* >= 16 in the reference (affine CUs) */
  uint8_t sixParam;     /* b6Param */
  uint8_t pad[7];
} vtmhip_affine_job;

/* both Sobel planes of n blocks (interior 3x3 Sobel, border samples replicated as the reference does) */
int vtmhip_affine_sobel_batch_dev( vtmhip_ctx *ctx, const int16_t *d_predBase, int32_t *d_derivBase, const vtmhip_affine_job *d_jobs, int n );
/* d_equalCoeff: n x [7][7] int64, ACCUMULATED into (the reference zeroes pEqualCoeff before the call); rows 1..np, columns 0..np are written */
int vtmhip_affine_equal_coeff_batch_dev( vtmhip_ctx *ctx, const int16_t *d_resiBase, const int32_t *d_derivBase, const vtmhip_affine_job *d_jobs, int n,
                                         int64_t *d_equalCoeff );

/* ---- affine motion estimation: InterSearch::xAffineMotionEstimation for one (PU, list, refIdx) per job ----------------------------------
 * (InterSearch.cpp:5340-5775) = the first prediction at the (clipped, AMVR-rounded) start model, up to 7 gradient iterations (error -> Sobel ->
 * normal equations -> solveEqual :5215-5284 -> control-point update -> InterPrediction::xPredAffineBlk :856-1232 -> SATD / SAD + xCalcAffineMVBits
 * :3067-3085) and the control-point refinement (:5655-5765), one workgroup per job from start to end: the fp64 steps run on the device in IEEE
 * double.  Covered: cu.imv 0 / 1 / 2, with AffineAmvrEncOpt too (imv 2: xDetermineBestMvp over the job's AMVP list); BCW weights (bcwWeight); PROF as the
 * caller's flags say.  Without an AMVP list in the job the predictor acMvPred and the AMVP index do not change, so the result is the model, its bits and cost. */
typedef struct
{
  int64_t  orgOff, refOff;          /* PU top-left in the original plane / the same position (MV 0,0) in the reference plane */
  int64_t  otherPredOff;            /* bi: the other list's prediction inside d_otherPredBase */
  int64_t  predOff;                 /* vtmhip_xPredAffineBlk_batch_dev only: where the prediction block goes inside d_dstBase */
  int32_t  orgStride, refStride, otherPredStride, predStride;
  int16_t  puX, puY, width, height; /* 16..128 */
  uint8_t  sixParam;                /* cu.affineType == AFFINEMODEL_6PARAM */
  uint8_t  interDir;                /* pu.interDir as isSubblockVectorSpreadOverLimit sees it */
  uint8_t  imv, bi;
  uint8_t  useSatd;                 /* !slice.getDisableSATDForRD() */
  uint8_t  useAffineType;           /* sps.getUseAffineType(): iteration counts :5470-5483 */
  uint8_t  amvrEncOpt;              /* m_pcEncCfg->getUseAffineAmvrEncOpt() */
  uint8_t  lowDelayRounds;          /* m_pcEncCfg->getIntraPeriod() == -1 */
  uint8_t  profAllowed;             /* sps.getUsePROF() && !m_skipPROF && !picHeader.getDisProfFlag() */
  uint8_t  profNeedsLargeGrad;      /* m_encOnly && !slice.getCheckLDC() */
  uint8_t  profIsBi;                /* m_isBi */
  int8_t   bcwWeight;               /* bi: getBcwWeight( cu.BcwIdx, searched list ); 0 or 4 = default (target 2*org - otherPred, distortion weight 0.5), else the weighted target
                                       of Buffer.h:417-460 and the distortion weight |w| / 8 */
  int32_t  mvPred[3][2];            /* acMvPred */
  int32_t  mv[3][2];                /* acMv on entry */
  uint32_t bits;                    /* ruiBits on entry */
  uint32_t pad1;
  double   motionLambda;
  uint64_t hevcCost;                /* m_hevcCost: the refinement stage runs when the best cost so far <= AFFINE_ME_LIST_MVP_TH * hevcCost */
  /* cu.imv == 2 with AffineAmvrEncOpt (ABI 6): xDetermineBestMvp (:7766-7785) re-picks the affine AMVP candidate at the start model and at every evaluation of the
   * gradient stage (:5444-5449, 5629-5634: acMvPred follows the pick even when the evaluation does not improve the cost; the refinement stage prices against the
   * predictor the LAST gradient evaluation left).  numAmvpCand == 0: no list given, the predictor never changes (every other mode). */
  int32_t  amvpCand[2][3][2];       /* aamvpi.mvCandLT / mvCandRT / mvCandLB of candidate i */
  uint32_t mvpIdxBits[2];           /* m_auiMVPIdxCost[i][aamvpi.numCand] */
  uint8_t  numAmvpCand;             /* aamvpi.numCand (1 or 2), 0: not given */
  uint8_t  mvpIdx;                  /* mvpIdx on entry: `bits` holds m_auiMVPIdxCost[mvpIdx][numCand] (dirBits = bits - that, :5359) */
  uint8_t  pad2[6];
} vtmhip_affine_me_job;

typedef struct
{
  int32_t  mv[3][2];                /* acMv */
  uint32_t bits;                    /* ruiBits */
  int32_t  iterations, refinements; /* predictions evaluated in the gradient stage / the refinement stage (statistics) */
  int32_t  mvpIdx;                  /* mvpIdx on return (changes only with an AMVP list in the job; acMvPred = that candidate, :5768-5770) */
  uint64_t cost;                    /* ruiCost */
} vtmhip_affine_me_out;

int vtmhip_xAffineMotionEstimation_batch_dev( vtmhip_ctx *ctx, const vtmhip_pic_params *pic, const int16_t *d_orgBase, const int16_t *d_refBase,
                                              const int16_t *d_otherPredBase, const vtmhip_affine_me_job *d_jobs, int n, int maxWidth, int maxHeight,
                                              vtmhip_affine_me_out *d_results );
/* The same call for a batch that may hold bi jobs under a CU-level BCW weight (vtmhip_affine_me_job::bcwWeight): a weight of -2 makes the search target -4 org + 5 pred, whose
 * differences leave the packed 16-bit Hadamard levels of the <= 10-bit kernel, so those jobs run in the 32-bit variant, launched beside the packed one (each job belongs to
 * exactly one of the two).  Results as above. */
int vtmhip_xAffineMotionEstimation_bcw_batch_dev( vtmhip_ctx *ctx, const vtmhip_pic_params *pic, const int16_t *d_orgBase, const int16_t *d_refBase,
                                                  const int16_t *d_otherPredBase, const vtmhip_affine_me_job *d_jobs, int n, int maxWidth, int maxHeight,
                                                  vtmhip_affine_me_out *d_results );
/* InterPrediction::xPredAffineBlk, luma, uni-directional (rounded and clipped; PROF as flagged) at the jobs' `mv` models */
int vtmhip_xPredAffineBlk_batch_dev( vtmhip_ctx *ctx, const vtmhip_pic_params *pic, const int16_t *d_refBase, int16_t *d_dstBase,
                                     const vtmhip_affine_me_job *d_jobs, int n, int maxWidth, int maxHeight );

/* ---- symmetric MVD search (SMVD) of predInterSearch (InterSearch.cpp:2656-2790) -----------------------------------------------------
 * One job = one PU with its two symmetric reference pictures: [0] the searched list (list 0 in predInterSearch :2662), [1] the mirrored list.
 *   op VTMHIP_SMVD_COST      InterSearch::xGetSymmetricCost (:4341-4391): cost = floor( fWeight * HAD-or-SAD( clip?( 2 * org - predA( mvCur ) ), predB( mvTar ) ) ),
 *                            each vector clipped (clipMv), integer vectors = the reconstruction, others xPredInterBlk (uni-directional, rounded, clipped);
 *                            BCW weights other than the default use removeWeightHighFreq and fWeight = |w| / 8 (xGetMEDistortionWeight :7666-7676)
 *   op VTMHIP_SMVD_ME        InterSearch::xSymmetricMotionEstimation (:4506-4518) with xSymmeticRefineMvSearch (:4393-4503): 8 >> imv diamond rounds and one
 *                            cross round of one AMVR step around mvCur, the mirrored vector predSym[1] - ( mv - predSym[0] ); in / out mvCur, mvTar, cost
 *   op VTMHIP_SMVD_CHECK_MVP InterSearch::symmvdCheckBestMvp (:7787-7886) for curMv = mvCur: every (i, j) of the two AMVP lists (skip != 0: but the current
 *                            pair); in / out predSym, mvpIdxSym, cost
 *   op VTMHIP_SMVD_SEARCH    the whole block :2656-2790: shortened AMVP lists (:2668-2671), best predictor pair, the distinct start vectors (starts[0..numFixed)
 *                            as they are = cMvHevcTemp, cMvTemp[, cMvBi]; the rest = m_uniMvList entries newest first, rounded to the AMVR precision, while
 *                            fewer than 5 are collected), symmvdCheckBestMvp per start, the search, the final predictor check, + getCost( modeBits );
 *                            out mvCur, mvTar, predSym, mvpIdxSym, cost (= symCost, to be compared with uiCostBi by the caller)
 * No MCTS constraint, no weighted prediction / RPR / wrap-around (the host keeps those PUs). */
#define VTMHIP_SMVD_COST 0
#define VTMHIP_SMVD_ME 1
#define VTMHIP_SMVD_CHECK_MVP 2
#define VTMHIP_SMVD_SEARCH 3
#define VTMHIP_SMVD_UNIFORM 0x100  /* or-ed into op: every job is exactly maxWidth x maxHeight (8x8 .. 16x16, bitDepth <= 10: the lane-per-tile kernel) */
#define VTMHIP_SMVD_MAX_START 18   /* cMvHevcTemp, cMvTemp, cMvBi + the 15 entries of m_uniMvList */
typedef struct
{
  int64_t  orgOff;                 /* origBuf.Y() inside d_orgBase */
  int64_t  refOff[2];              /* PU position with MV (0,0) inside d_refBase: [0] searched list, [1] mirrored list */
  int32_t  orgStride, refStride[2];
  int16_t  puX, puY, width, height;
  uint8_t  imv;                    /* cu.imv: 0 quarter, 1 integer, 2 four-sample, 3 half (alternative half-sample filter) */
  uint8_t  useSatd;                /* !slice.getDisableSATDForRD() */
  uint8_t  clipBiPred;             /* cfg ClipForBiPredMEEnabled */
  int8_t   bcwWeightTar;           /* getBcwWeight( cu.BcwIdx, mirrored list ): 0 or 4 = default */
  uint8_t  numCand[2];             /* AMVP lists of the two symmetric references */
  uint8_t  numStart, numFixed;     /* SEARCH: start vectors */
  uint8_t  skip;                   /* CHECK_MVP */
  uint8_t  pad_[3];
  int32_t  cand[2][2][2];          /* [list][i][hor / ver] */
  uint32_t mvpIdxBits[2];          /* m_auiMVPIdxCost[i][AMVP_MAX_NUM_CANDS] */
  uint32_t modeBits;               /* SEARCH: uiMbBits[2] + 1 + BCW index bits (:2782-2785) */
  double   motionLambda;
  int32_t  starts[VTMHIP_SMVD_MAX_START][2];
  /* in / out */
  int32_t  mvCur[2], mvTar[2];
  int32_t  predSym[2][2];          /* cMvPredSym */
  int32_t  mvpIdxSym[2];
  uint64_t cost;
  /* op VTMHIP_SMVD_SEARCH only: the state of the block at the points where the reference's code sits between two member calls (a host that replays predInterSearch's
   * own glue over device results -- INTEGRATION.md section 3.1 -- serves the members from these):
   *   [0] after the predictor-pair loop (:2675-2691): cost = the winning pair's xGetSymmetricCost (no rate), idx = the pair
   *   [1] after the start-vector loop (:2744-2763):   mv = cCurMvField.mv, idx = mvpIdxSym, cost = costStart
   *   [2] after xSymmetricMotionEstimation (:2770):   mv = cCurMvField.mv, cost = symCost as the member returns it (without mvpCost)
   *   [3] after the final predictor check (:2774-2777): idx = mvpIdxSym, cost = symCost (with mvpCost, before the mode bits) */
  struct { uint64_t cost; int32_t mv[2]; int32_t idx[2]; } trace[4];
} vtmhip_smvd_job;
int vtmhip_smvd_batch_dev( vtmhip_ctx *ctx, const vtmhip_pic_params *pic, const int16_t *d_orgBase, const int16_t *d_refBase, vtmhip_smvd_job *d_jobs, int n,
                           int maxWidth, int maxHeight, int op );
/* Which kernel vtmhip_smvd_batch_dev launches for a call with these arguments (uniform: VTMHIP_SMVD_UNIFORM is set), the one rule the call itself dispatches on:
 *   VTMHIP_SMVD_KERNEL_GENERAL_64 / _256   one workgroup of 64 / 256 lanes per PU, any size and bit depth (wavesPerPU = slots = pusPerWave = 0)
 *   VTMHIP_SMVD_KERNEL_TILE_GROUP          the lane-per-tile kernel, a PU inside one wave: wavesPerPU 0, slots = candidates of a pass evaluated at once (8 while the
 *                                          batch is at most eight eight-slot waves per compute unit, ceil( n / ( 64 / ( 8 * tiles ) ) ) <= 8 * CUs, else 4),
 *                                          pusPerWave = 64 / ( slots * tiles ), tiles = the PU's 8x8 tiles
 *   VTMHIP_SMVD_KERNEL_TILE_WORKGROUP      the lane-per-tile kernel, one PU per workgroup of wavesPerPU waves: slots 8, pusPerWave 1 (PUs per workgroup)
 * Host arithmetic, no device needed: ctx may be NULL (a device of 256 compute units).  VTMHIP_E_INVALID for the sizes and bit depths vtmhip_smvd_batch_dev refuses. */
#define VTMHIP_SMVD_KERNEL_GENERAL_64 0
#define VTMHIP_SMVD_KERNEL_GENERAL_256 1
#define VTMHIP_SMVD_KERNEL_TILE_GROUP 2
#define VTMHIP_SMVD_KERNEL_TILE_WORKGROUP 3
int vtmhip_smvd_launch_form( const vtmhip_ctx *ctx, int maxWidth, int maxHeight, int bitDepth, int uniform, int n, int *kernel, int *wavesPerPU, int *slots,
                             int *pusPerWave );
/* the reference's names for the four ops */
int vtmhip_xGetSymmetricCost_batch_dev( vtmhip_ctx *ctx, const vtmhip_pic_params *pic, const int16_t *d_orgBase, const int16_t *d_refBase, vtmhip_smvd_job *d_jobs,
                                        int n, int maxWidth, int maxHeight );
int vtmhip_xSymmetricMotionEstimation_batch_dev( vtmhip_ctx *ctx, const vtmhip_pic_params *pic, const int16_t *d_orgBase, const int16_t *d_refBase,
                                                 vtmhip_smvd_job *d_jobs, int n, int maxWidth, int maxHeight );
int vtmhip_symmvdCheckBestMvp_batch_dev( vtmhip_ctx *ctx, const vtmhip_pic_params *pic, const int16_t *d_orgBase, const int16_t *d_refBase, vtmhip_smvd_job *d_jobs,
                                         int n, int maxWidth, int maxHeight );

/* ================================================================================================================
 * (3) LEVEL-ORDER DRIVER SUPPORT -- whole functions per batch and the glue between them, decisions kept on the device
 * ============================================================================================================== */

/* ---- merge-candidate estimation: the SATD pre-selection of EncCu::xCheckRDCostMerge2Nx2N (hook B10) ---------------------------------------
 * (EncCu.cpp:2399-2440; the MMVD and CIIP candidate loops :2470-2549 use the same two steps).  For every candidate the reference runs
 * motionCompensation( pu, ..., luma ) -- plain uni / bi prediction, BDOF or DMVR (+ BDOF) by the candidate's motion -- and the Hadamard (or SAD)
 * distortion against the original block; the candidate's bits x sqrt(lambda) and the sorted insertion (updateCandList) stay with the host.
 * One call: the three job tables (candidates grouped by the kind of prediction; any may be empty) -> predictions into d_predBase + predOff (kept:
 * they are the encoder's acMergeBuffer) -> d_dist[nPlain + nBdof + nDmvr] in table order.  Jobs: epilogue 0; d_mvd as vtmhip_dmvr_batch_dev.
 * The MMVD candidates have an entry of their own, vtmhip_mmvd_cand_satd_batch_dev below: it derives them on the device and keeps no prediction. */
int vtmhip_merge_cand_satd_batch_dev( vtmhip_ctx *ctx, const vtmhip_pic_params *pic, const int16_t *d_orgBase, const int16_t *d_refBase, int16_t *d_predBase,
                                      const vtmhip_pred_job *d_plain, int nPlain, const vtmhip_pred_job *d_bdof, int nBdof, const vtmhip_dmvr_job *d_dmvr, int nDmvr,
                                      int32_t *d_mvd, int maxWidth, int maxHeight, int uniformSize, int useSatd, uint64_t *d_dist );

/* ---- MMVD merge candidates: the MMVD loop of the same pre-selection (EncCu.cpp:2524-2562, hook B10) -----------------------------------------
 * Per CU the reference walks up to MMVD_ADD_NUM = 64 candidates: MergeCtx::setMmvdMergeCandiInfo (ContextModelling.cpp:355-528) turns the index into a motion,
 * motionCompensation predicts the luma block into ONE buffer (singleMergeTempBuffer, swapped into the list only on an insertion) and the Hadamard (or SAD) against
 * the original is the candidate's distortion.  Here one job is one CU with its (up to) two base candidates; the 64 motions are derived on the device, the plain
 * predictions never leave the kernel, and what comes back per (job, candidate) is the distortion and the record the host needs for xCalcPuMeBits, spanMotionInfo and
 * to predict a survivor again through the motion-compensation entries (the RD stage does that with mmvdEncOptMode 0, EncCu.cpp:2668-2740).
 *
 * Candidate index (ContextModelling.cpp:367-373): cand = base * 32 + step * 4 + pos, base 0 / 1, step 0 .. 7, pos 0 .. 3.  The offset is ( 1 << step ) << 2 in 1/16
 * units, << 2 more under picHeader.getDisFracMMVD() (:374-378); pos 0: +hor, 1: -hor, 2: +ver, 3: -ver.  A bi base gives the offset to the list whose picture is
 * further away (or to both on equal POC differences) and the other list the offset scaled by PU::getDistScaleFactor / Mv::scaleMv, or -- either picture long-term --
 * copied / mirrored by the sign of ( poc1 - cur ) * ( poc0 - cur ) (:382-452); a uni base moves its one list (:453-500).  The lists in use go through
 * clipToStorageBitDepth (:518-524) and PU::restrictBiPredMergeCandsOne (:527, UnitTools.cpp:3262: width + height == 12 makes a bi candidate uni list 0 with the
 * default BCW weight).  The loop (EncCu.cpp:2528-2534) tests 64 candidates when numValidMergeCand > 1, else 32 -- numBase 2 / 1 here -- and skips step >=
 * MmvdDisNum -- numSteps.
 * The prediction (InterPrediction.cpp:527-572): BDOF iff bdofAllowed, the restricted candidate is bi, PU::isBiPredFromDifferentDirEqDistPoc (neither picture
 * long-term, opposite sides, equal distance), w >= 8, h >= 8, w * h >= 128, default BCW weight and step <= 2 (mmvdEncOptMode 2 for refineStep > 2 switches BDOF
 * off, :563-565); DMVR never (PU::checkDMVRCondition excludes mmvdMergeFlag).  Otherwise plain: uni, addAvg, or addWeightedAvg under the base's BCW weight; a bi
 * candidate whose two lists name the same picture (equal pocDiff) with equal vectors is predicted from list 0 alone (xCheckIdenticalMotion :240-272, :1564).  The
 * vector a prediction uses is clipMv of the stored one at the CU's luma position (Mv.cpp:56-74); the record carries the stored one. */
typedef struct
{
  int32_t mv[2][2];             /* mmvdBaseMv[base][list].mv: [list][hor, ver], internal 1/16 precision */
  int64_t refOff[2];            /* block position with MV (0,0) in the list-0 / list-1 reference plane, as vtmhip_pred_job (unused where refIdx < 0) */
  int32_t refStride[2];
  int32_t pocDiff[2];           /* slice.getRefPOC( list, refIdx ) - slice.getPOC() */
  int8_t  refIdx[2];            /* mmvdBaseMv[base][list].refIdx; -1: the list is not used.  Not ( -1, -1 ) */
  uint8_t longTerm[2];          /* slice.getRefPic( list, refIdx )->longTerm */
  uint8_t useAltHpelIf;         /* mergeCtx.mmvdUseAltHpelIf[base] */
  int8_t  bcwWeightL1;          /* g_BcwWeights[mergeCtx.BcwIdx[base]] in {-2, 3, 4, 5, 10}: the list-1 weight of vtmhip_add_weighted_avg_batch_dev; used when the base is bi */
  uint8_t pad[2];
} vtmhip_mmvd_base;

typedef struct
{
  int64_t orgOff;               /* the CU's luma block in the original plane */
  int32_t orgStride;
  int32_t posX, posY;           /* cu.lumaPos(): what clipMv sees */
  int16_t width, height;        /* 4 .. 128, powers of two, not 4 x 4 */
  uint8_t bitDepth;             /* 8 .. 12 */
  uint8_t numBase;              /* 1: numValidMergeCand <= 1, candidates 0 .. 31; 2: all 64 */
  uint8_t numSteps;             /* m_pcEncCfg->getMmvdDisNum(): 1 .. 8, candidates of step >= numSteps are not tested */
  uint8_t disFracMmvd;          /* picHeader.getDisFracMMVD() */
  uint8_t bdofAllowed;          /* sps.getBDOFEnabledFlag() && !picHeader.getDisBdofFlag(), no weighted prediction, no scaled reference */
  uint8_t pad[3];
  vtmhip_mmvd_base base[2];     /* base[1] is not read when numBase == 1 */
} vtmhip_mmvd_job;

enum { VTMHIP_MMVD_NOT_TESTED = 0, VTMHIP_MMVD_PLAIN = 1, VTMHIP_MMVD_BDOF = 2, VTMHIP_MMVD_NUM_CAND = 64 };

typedef struct
{
  int32_t mv[2][2];             /* pu.mv as setMmvdMergeCandiInfo leaves it (stored vector: before clipMv); ( 0, 0 ) on an unused list */
  int8_t  refIdx[2];            /* pu.refIdx; -1 on an unused list */
  uint8_t interDir;             /* pu.interDir after restrictBiPredMergeCandsOne: 1, 2 or 3 */
  int8_t  bcwWeightL1;          /* the weight of cu.BcwIdx: the base's when interDir == 3, else 4 */
  uint8_t useAltHpelIf;         /* cu.imv == IMV_HPEL */
  uint8_t kind;                 /* VTMHIP_MMVD_NOT_TESTED (the loop skips the candidate: every other field 0, refIdx -1), _PLAIN, _BDOF */
  uint8_t pad[2];
} vtmhip_mmvd_cand;

int vtmhip_mmvd_struct_size( int which );   /* sizeof() of 0 vtmhip_mmvd_job, 1 vtmhip_mmvd_cand, 2 vtmhip_mmvd_base; -1 otherwise */

/* The derivation alone, as host arithmetic (no device, no context): out[64] as the device leaves d_cand, predMv[cand][list][hor, ver] the clipped vectors the
 * predictions use (0 on an unused list and where kind == 0).  VTMHIP_E_INVALID for a job the table predicate rejects (below) or pic outside its contract. */
int vtmhip_mmvd_cands_host( const vtmhip_mmvd_job *job, const vtmhip_pic_params *pic, vtmhip_mmvd_cand out[64], int32_t predMv[64][2][2] );

/* One call per batch of CUs: d_cand[n * 64] and d_dist[n * 64] at [job * 64 + cand]; d_dist is the SATD (useSatd != 0: the tile rules of xGetHADs) or SAD of the
 * candidate's luma prediction against the original, UINT64_MAX where kind == VTMHIP_MMVD_NOT_TESTED.  maxWidth / maxHeight bound the CU sizes of the batch (lanes per
 * block as vtmhip_mc_lanes_per_block).  The plain candidates run in one fused kernel (derivation, both predictions and the distortion, nothing but the cost and the
 * record stored); the BDOF candidates (at most 24 per CU) are expanded into vtmhip_pred_job rows and run through vtmhip_bdof_batch_dev and the distortion call over
 * an internal workspace.  VTMHIP_MMVD_FUSED=0 in the environment sends every candidate through that expansion (vtmhip_motion_compensation_batch_dev for the plain
 * ones): a second route to the same tables, and the default for batches whose blocks take a workgroup each (maxWidth x maxHeight above 1024 samples), where it measured faster (VTMHIP_MMVD_FUSED=1: the fused
 * kernel there too).  A BDOF candidate of a base with useAltHpelIf is predicted with the regular half-sample filter, as vtmhip_bdof_batch_dev predicts every PU.
 * The job table is read back (n * sizeof( vtmhip_mmvd_job ) bytes, one stream synchronisation; never under stream capture) and checked before anything is launched; a
 * malformed job REJECTS THE WHOLE CALL with VTMHIP_E_INVALID and nothing written: sides outside 4 .. 128 / not powers of two / 4 x 4 / above maxWidth x maxHeight,
 * numBase outside 1 .. 2, numSteps outside 1 .. 8, a base in use with refIdx ( -1, -1 ), bitDepth outside 8 .. 12 or different from pic->bitDepth, a stride below
 * the width, a BCW weight outside {-2, 3, 4, 5, 10}.  Reference planes as described under VTMHIP_PLANE_SLACK. */
int vtmhip_mmvd_cand_satd_batch_dev( vtmhip_ctx *ctx, const vtmhip_pic_params *pic, const int16_t *d_orgBase, const int16_t *d_refBase, const vtmhip_mmvd_job *d_jobs,
                                     int n, int maxWidth, int maxHeight, int useSatd, vtmhip_mmvd_cand *d_cand, uint64_t *d_dist );

/* ---- CIIP merge candidates: the combined inter-intra loop of the same pre-selection (EncCu.cpp:2460-2523, hook B10) and its RD-stage blend (:2706-2735) ------
 * Eligible (EncCu.cpp:2335-2339): sps.getUseCiip(), w * h >= 64, w < 128, h < 128 -- sides 4 .. 64, every combination of at least 64 samples.  The loop tests the
 * first min( min( NUM_MRG_SATD_CAND = 4, numValidMergeCand ), 4 ) entries of RdModeList after the regular loop: at most four per CU.
 *   inter part   acMergeTmpBuffer[cand]: the predBufWOBIO of the regular loop's motionCompensation -- the PLAIN prediction from the candidate's stored vectors:
 *                uni = the rounded and clipped block, bi = the default-weight addAvg of the two 14-bit blocks; no BDOF, no DMVR refinement
 *                (InterPrediction.cpp:594-599), no BCW weight (:1368), identical motion on both lists from list 0 alone (:1564-1572: the caller sends mode 0)
 *   intra part   once per CU: planar, multiRefIdx 0, through initIntraPatternChType + predIntraAng under the regular rules (nothing tests ciipFlag): the [1 2 1]
 *                line filter (refFilterFlag = w * h > 32: always for a CIIP luma block) and PDPC
 *   blend        IntraPrediction::geneWeightedPred (IntraPrediction.cpp:682-722): wIntra = 3 / 2 / 1 when both / one / none of the PUs left of the bottom-left
 *                sample and above the top-right sample exist and are intra; dst = ( ( 4 - wIntra ) * inter + wIntra * intra + 2 ) >> 2, no clip
 *   LMCS         (slice flag and CTU flag) the inter luma block goes through the forward LUT before the blend, the blended block through the inverse LUT before
 *                the distortion; the intra lines are reconstruction samples: mapped already
 *   cost         distParam.distFunc -- SATD, or SAD under getDisableSATDForRD -- against the original luma block
 * The bits, updateCandList and the MRG_FAST_RATIO cut stay with the host.  Outside: explicit weighted prediction, scaled references, 4:2:2 and 4:4:4. */

/* The reshaper's inverse LUT (1 << lumaBD entries) for callers that do not use the weighted SSE; ordering and lifetime as vtmhip_set_lmcs_fwd_lut (copied before
 * the call returns, visible to every later call on the context).  The slot is its own: vtmhip_set_luma_level_weights keeps the inverse LUT of the DF_SSE_WTD
 * entries in another one, and neither setter touches the other's, so a caller of both sets the table twice. */
int vtmhip_set_lmcs_inv_lut( vtmhip_ctx *ctx, const int16_t *invLut, int lumaBD );

enum { VTMHIP_CIIP_MAX_CAND = 4 };

typedef struct
{
  int64_t refOff[2];            /* modes 0 .. 2: block position with MV (0,0) in the list-0 / list-1 reference plane inside d_refBase, as vtmhip_pred_job */
  int64_t srcOff;               /* mode 3: the inter luma block inside d_predBase */
  int64_t keepOff;              /* -1, or where the blended luma block IN THE MAPPED DOMAIN is written inside d_predBase, stride width: the RD stage's luma prediction */
  int32_t refStride[2];
  int32_t mv[2][2];             /* [list][hor, ver], internal 1/16 precision: the vector the prediction uses, clipMv already applied (as vtmhip_pred_job) */
  int32_t srcStride;            /* mode 3 */
  uint8_t mode;                 /* 0: list 0, 1: list 1, 2: bi (default-weight addAvg), 3: the inter block is given at srcOff / srcStride -- what a caller holds after
                                   vtmhip_merge_cand_satd_batch_dev for a candidate whose kept prediction is already the plain one (no BDOF, no DMVR, default BCW) */
  uint8_t useAltHpelIf;
  uint8_t pad[2];
} vtmhip_ciip_cand;

typedef struct
{
  int64_t lineOff;              /* inside d_lineBase: the top line of 2W + 1 samples, index 0 = the corner, then the left line of 2H + 1, index 0 = the same corner
                                   (the lines of a vtmhip_intra_block with multiRefIdx 0) */
  int64_t orgOff;               /* the CU's luma block in the original plane */
  int32_t orgStride;
  int16_t width, height;        /* 4 .. 64 each, width * height >= 64 */
  uint8_t bitDepth;             /* 8 .. 12 */
  uint8_t leftIntra;            /* the PU at bottomLeft.offset( -1, 0 ) exists and is intra */
  uint8_t aboveIntra;           /* the PU at topRight.offset( 0, -1 ) exists and is intra */
  uint8_t lmcs;                 /* slice.getLmcsEnabledFlag() && reshaper.getCTUFlag() */
  uint8_t numCand;              /* 1 .. 4 */
  uint8_t pad[3];
  vtmhip_ciip_cand cand[VTMHIP_CIIP_MAX_CAND];
} vtmhip_ciip_job;

typedef struct
{
  int64_t lineOff;              /* as vtmhip_ciip_job, for this block's width and height (a chroma block: the lines of that plane) */
  int64_t predOff;              /* the inter block inside d_predBase; the blend is written over it */
  int32_t predStride;
  int16_t width, height;        /* luma: as vtmhip_ciip_job; chroma: width 4 .. 32, height 2 .. 32, at least 16 samples (the 4:2:0 block of a CIIP CU).  A WIDTH of 2 is
                                   malformed: the caller keeps the inter block, as the reference does (EncCu.cpp:2718); a height of 2 is blended, without PDPC */
  uint8_t bitDepth;
  uint8_t chroma;               /* DM_CHROMA of a planar luma: planar without the line filter, PDPC on */
  uint8_t leftIntra, aboveIntra;   /* the LUMA neighbours, for chroma blocks too */
  uint8_t mapFwd;               /* luma only: the inter block goes through the forward LUT first (the result stays in the mapped domain) */
  uint8_t pad[3];
} vtmhip_ciip_blend_job;

int vtmhip_ciip_struct_size( int which );   /* sizeof() of 0 vtmhip_ciip_job, 1 vtmhip_ciip_cand, 2 vtmhip_ciip_blend_job; -1 otherwise */

/* One CU as host arithmetic (no device, no context).  inter[k]: the plain inter luma block of candidate k, width x height with stride width, for EVERY mode (the
 * host has no interpolation entry; refOff / mv / srcOff are not read).  fwdLut / invLut: needed iff job->lmcs.  blend: numCand blocks of width * height samples --
 * the blended blocks in the mapped domain (what keepOff receives); satd[k] / sad[k]: both costs of candidate k against the original, UINT64_MAX from numCand on.
 * VTMHIP_E_INVALID for a job the table predicate rejects (below, with maxWidth = maxHeight = 64) or a missing pointer. */
int vtmhip_ciip_host( const vtmhip_ciip_job *job, const int16_t *lineBase, const int16_t *orgBase, const int16_t *const inter[VTMHIP_CIIP_MAX_CAND], const int16_t *fwdLut,
                      const int16_t *invLut, int16_t *blend, uint64_t satd[VTMHIP_CIIP_MAX_CAND], uint64_t sad[VTMHIP_CIIP_MAX_CAND] );
/* vtmhip_ciip_blend_batch_dev for one job on the host; fwdLut is needed iff job->mapFwd.  VTMHIP_E_INVALID for a job the device would skip. */
int vtmhip_ciip_blend_host( const vtmhip_ciip_blend_job *job, const int16_t *lineBase, int16_t *predBase, const int16_t *fwdLut );

/* One call per batch of CUs, one fused kernel: per CU the planar block with PDPC is formed once in LDS, and per candidate the inter block (motion compensation inside
 * the kernel for modes 0 .. 2, a copy for mode 3), the forward LUT, the blend, the optional kept store, the inverse LUT and the distortion run from LDS.  Apart from
 * the kept blocks no prediction sample goes to global memory.  d_dist[job * 4 + cand] = the SATD (useSatd != 0: the tile rules of xGetHADs) or SAD; a slot at or
 * beyond numCand, and every slot of a skipped job, holds UINT64_MAX.  maxWidth x maxHeight (a well-formed CIIP size) bounds the CUs of the batch; lanes per CU as
 * vtmhip_mc_lanes_per_block.
 * The job table is never read back and the stream is never synchronised: the call only queues work and may run under stream capture.  A job that fails the
 * predicate is skipped ON THE DEVICE -- nothing is read through it, its four costs are UINT64_MAX and no kept block is written: sides outside the CIIP set or
 * above maxWidth x maxHeight, bitDepth outside 8 .. 12, numCand outside 1 .. 4, a mode above 3, a stride (orgStride, the refStride of a list in use, srcStride of
 * mode 3) below the width, lmcs set in a call whose lmcs argument is 0, or lmcs set with a bitDepth that is not the LUTs'.
 * lmcs != 0: jobs may set their lmcs flag; the call fails with VTMHIP_E_INVALID before launching anything when either LUT (vtmhip_set_lmcs_fwd_lut,
 * vtmhip_set_lmcs_inv_lut) is missing or their depths differ.  A LUT index outside the table is held at its ends.  d_predBase may be NULL when no job has a
 * mode-3 candidate or a kept block.  Reference planes as described under VTMHIP_PLANE_SLACK. */
int vtmhip_ciip_cand_satd_batch_dev( vtmhip_ctx *ctx, const int16_t *d_refBase, const int16_t *d_lineBase, const int16_t *d_orgBase, int16_t *d_predBase,
                                     const vtmhip_ciip_job *d_jobs, int n, int maxWidth, int maxHeight, int useSatd, int lmcs, uint64_t *d_dist );

/* geneWeightedPred in place for n blocks: the RD stage's Cb and Cr blocks (chroma planar, the luma neighbour weights), and luma where the block was not kept.  Luma
 * and chroma jobs mix freely.  Lanes per job follow the rule of vtmhip_intra_pred_batch_dev (vtmhip_intra_lanes_per_job of the largest well-formed block; a small
 * kernel finds it: no read-back, no synchronisation).  A malformed job is skipped on the device and its block left as it is: a size outside what vtmhip_ciip_blend_job lists, a
 * bitDepth outside 8 .. 12, predStride below the width, mapFwd on a chroma job, mapFwd without a forward LUT of the job's depth. */
int vtmhip_ciip_blend_batch_dev( vtmhip_ctx *ctx, const int16_t *d_lineBase, int16_t *d_predBase, const vtmhip_ciip_blend_job *d_jobs, int n );

/* ---- GEO merge candidates: EncCu::xCheckRDCostMergeGeo2Nx2N up to its RD stage (EncCu.cpp:2811-3031, hook B10) ------------------------------------------------
 * Eligible: sides 8, 16, 32 or 64 with w < 8h and h < 8w (14 shapes).  Per CU the reference runs, in this order: numCand = sps.getMaxNumGeoCand() uni-predictions
 * kept as 14-bit blocks (geoBuffer), their rounded copies' whole-block SADs, 64 x numCand masked SADs (sadLarge; sadSmall = sadWhole - sadLarge), the cost filter
 * over 64 x numCand x ( numCand - 1 ) (split, candidate pair) combinations, the sort, and for the first min( passed, 60 ) of the list the blend of the two 14-bit
 * blocks with the distortion (SATD, or SAD under getDisableSATDForRD) against the original.
 *   weights      a plane entry is Clip3( 0, 8, ( 32 + wIdx + 4 ) >> 3 ), a mask entry wIdx > 0, with wIdx in closed form per sample: no plane is uploaded
 *   first pass   in double, exactly as written: side cost = (double) sad + (double) ( cand + 1 ) * sqrtLambda; bestWholeBlkCost from the first strict minimum of
 *                the whole-block SADs; a combination is dropped when cost0 + cost1 > bestWholeBlkCost and otherwise kept with + 6 * sqrtLambda
 *   list order   ascending cost; ties by splitDir, then by index in the pair order m_GeoModeTest -- a total order and one valid outcome of the reference's unstable
 *                std::sort; this is the project's rule
 * With the host: PU::getGeoMergeCandidates, the all-duplicates early return (such a CU is not sent), MCTS, the second-pass cost from dist and the bits,
 * updateCandList and the MRG_FAST_RATIO / best-SATD cuts, spanGeoMotionInfo, 4:2:2 and 4:4:4. */
enum { VTMHIP_GEO_MAX_CAND = 6, VTMHIP_GEO_MAX_TRY = 60 };

typedef struct
{
  int64_t refOff;               /* block position with MV (0,0) in the plane of the ONE list the candidate uses, inside d_refBase */
  int64_t keepOff;              /* -1, or where the candidate's 14-bit luma block is written inside d_predBase, stride width: the encoder's geoBuffer */
  int32_t refStride;
  int32_t mv[2];                /* hor, ver, internal 1/16 precision, clipMv already applied (as vtmhip_ciip_cand); cu.imv is 0: no alternative half-sample filter */
  int32_t pad;
} vtmhip_geo_cand;

typedef struct
{
  int64_t orgOff;               /* the CU's luma block in the original plane */
  double  sqrtLambda;           /* RdCost::getMotionLambda(): finite, not negative */
  int32_t orgStride;
  int16_t width, height;        /* one of the 14 shapes */
  uint8_t bitDepth;             /* 8 .. 12 */
  uint8_t numCand;              /* 2 .. 6 */
  uint8_t pad[6];
  vtmhip_geo_cand cand[VTMHIP_GEO_MAX_CAND];
} vtmhip_geo_job;

typedef struct
{
  double   cost;                /* the first-pass cost of the list */
  uint64_t dist;                /* the blended luma block against the original: SATD (the tile rules of xGetHADs) or SAD; UINT64_MAX in an unused slot */
  uint8_t  splitDir, cand0, cand1;
  uint8_t  pad[5];
} vtmhip_geo_combo;

typedef struct
{
  uint64_t sadWhole[VTMHIP_GEO_MAX_CAND];   /* UINT64_MAX from numCand on */
  int32_t  numPassed;                       /* combinations that passed the filter */
  int32_t  numTested;                       /* min( numPassed, 60 ) */
  vtmhip_geo_combo combo[VTMHIP_GEO_MAX_TRY];   /* list order; from numTested on: dist UINT64_MAX, every other field 0 */
} vtmhip_geo_result;

typedef struct
{
  int64_t src0Off, src1Off;     /* the two 14-bit blocks of this plane inside d_srcBase */
  int64_t dstOff;               /* inside d_dstBase */
  int32_t src0Stride, src1Stride, dstStride;
  int16_t width, height;        /* the CU's LUMA size, for chroma jobs too: a chroma job blends ( width / 2 ) x ( height / 2 ) samples */
  uint8_t splitDir;             /* 0 .. 63 */
  uint8_t chroma;               /* 0: luma; 1: a 4:2:0 Cb / Cr block (the plane is read two entries apart) */
  uint8_t bitDepth;
  uint8_t pad[5];
} vtmhip_geo_cu_blend_job;

int vtmhip_geo_struct_size( int which );   /* sizeof() of 0 vtmhip_geo_job, 1 vtmhip_geo_cand, 2 vtmhip_geo_combo, 3 vtmhip_geo_result, 4 vtmhip_geo_cu_blend_job; -1 otherwise */
/* lanes that work on one CU of a vtmhip_geo_cand_satd_batch_dev call: 64 up to 1024 samples, 256 above; 0 when maxWidth x maxHeight is none of the 14 shapes */
int vtmhip_geo_lanes_per_job( int maxWidth, int maxHeight );

/* The weights (chroma = 0: width x height, chroma = 1: ( width / 2 ) x ( height / 2 ), stride = that width) and the SAD mask (always luma, width x height) of one
 * split of a width x height CU, from the closed form.  Either output may be NULL.  VTMHIP_E_INVALID for a size outside the 14 shapes or a splitDir outside 0 .. 63. */
int vtmhip_geo_tables_host( int splitDir, int width, int height, int chroma, int16_t *weightOut, int16_t *maskOut );

/* One CU as host arithmetic (no device, no context) from given 14-bit blocks: pred[k] is candidate k's block, width x height with stride width (refOff / mv are not
 * read; a keepOff is ignored).  result: as the device leaves it with useSatd.  sadSplit (may be NULL): 64 x 6 sadLarge at [split * 6 + cand], UINT64_MAX from numCand
 * on.  blend (may be NULL): result->numTested blocks of width * height samples, in list order.  VTMHIP_E_INVALID for a job the table predicate rejects (with
 * maxWidth = maxHeight = 64) or a missing pointer: nothing is written then. */
int vtmhip_geo_host( const vtmhip_geo_job *job, const int16_t *orgBase, const int16_t *const pred[VTMHIP_GEO_MAX_CAND], int useSatd, vtmhip_geo_result *result,
                     uint64_t *sadSplit, int16_t *blend );

/* One call per batch of CUs, one fused kernel: per CU the candidates' motion compensation as 14-bit intermediates into LDS, the kept stores, the whole-block and the
 * 64 x numCand masked SADs of the rounded blocks (the mask from the closed form), the filter and the ordered list in LDS, and per listed combination the blend with
 * closed-form weights and the distortion straight from LDS.  Apart from the kept blocks and the result tables no sample goes to global memory.
 * d_result[job]; d_sadSplit (may be NULL): [job * 384 + split * 6 + cand], UINT64_MAX from numCand on.  maxWidth x maxHeight (one of the 14 shapes) bounds the CUs
 * of the batch; lanes per CU as vtmhip_geo_lanes_per_job.
 * The job table is never read back and the stream is never synchronised: the call only queues work and may run under stream capture (the first call of a process
 * on a device whose bound is above 1024 samples also raises the kernel's dynamic-LDS limit, once; that is no stream operation).  A job that fails the
 * predicate is skipped ON THE DEVICE -- nothing is read through it, numPassed and numTested are 0, sadWhole, every dist and every d_sadSplit entry of the job are
 * UINT64_MAX, every other field 0 and no kept block is written: a size outside the 14 shapes or above maxWidth x maxHeight, bitDepth outside 8 .. 12, numCand
 * outside 2 .. 6, a stride (orgStride, a candidate's refStride) below the width, a sqrtLambda that is not finite or is negative, a keepOff >= 0 with d_predBase
 * NULL.  Reference planes as described under VTMHIP_PLANE_SLACK. */
int vtmhip_geo_cand_satd_batch_dev( vtmhip_ctx *ctx, const int16_t *d_refBase, const int16_t *d_orgBase, int16_t *d_predBase, const vtmhip_geo_job *d_jobs, int n,
                                    int maxWidth, int maxHeight, int useSatd, vtmhip_geo_result *d_result, uint64_t *d_sadSplit );

/* weightedGeoBlk for n blocks with closed-form weights: the RD stage's luma, Cb and Cr blocks of the survivors (EncCu.cpp:3023-3031, :3073), from 14-bit blocks --
 * kept luma blocks, chroma blocks of vtmhip_mc_batch_dev with bi = 1, chroma = 1.  Luma and chroma jobs mix freely; d_srcBase and d_dstBase may be the same array when
 * no job's destination overlaps another job's source.  A malformed job is skipped on the device and its destination left as it is: a size outside the 14 shapes, a
 * splitDir above 63, chroma above 1, bitDepth outside 8 .. 12, a stride below the block's width.  Queues work only. */
int vtmhip_geo_blend_batch_dev( vtmhip_ctx *ctx, const int16_t *d_srcBase, int16_t *d_dstBase, const vtmhip_geo_cu_blend_job *d_jobs, int n );

/* ================================================================================================================
 * (4) LEVEL-ORDER predInterSearch -- InterSearch::predInterSearch (InterSearch.cpp:2245-3065, translational part: cu.imv 0, default
 *     BCW weight, no SMVD / affine) for ALL PUs of one block size at once, on top of the batched calls above
 * ==============================================================================================================
 * One PU of the reference runs: for every (list, refIdx): xEstimateMvPredAMVP, xMotionEstimation, xCheckBestMVP, best reference per list
 * (:2354-2450); B slices: the list with the larger cost is refined against the other list's prediction for every refIdx (one iteration:
 * FASTINTERSEARCH_MODE1, :2544-2556), xCheckBestMVP, then the uni / bi decision (:2846-2893).  A level-order driver issues the same steps as
 * batched launches over all PUs of a level; these helpers are the per-PU arithmetic in between (one thread per PU / row), so that nothing
 * returns to the host.  Rows of the uni tables are ordered (list, refIdx)-major, PU-minor: row = (list ? numRef[0] : 0) + refIdx) * numPU + pu;
 * rows of the bi tables: refIdx * numPU + pu.  What stands in for the CU recursion: the two AMVP candidates of a row are the enclosing
 * parent block's vector for the same (list, refIdx) and the zero vector (the reference derives them from neighbouring CUs). */
#define VTMHIP_MAX_REF 4

typedef struct
{
  int32_t  mvHor, mvVer;           /* cMvTemp[list][refIdx] */
  int32_t  mvPredHor, mvPredVer;   /* cMvPred[list][refIdx] after xCheckBestMVP */
  int32_t  mvpIdx;                 /* aaiMvpIdx */
  uint32_t bits;                   /* uiBitsTemp */
  uint64_t cost;                   /* uiCostTemp */
} vtmhip_pis_row;

typedef struct
{
  uint64_t cost[2];                /* uiCost[list] (max when the list is empty) */
  uint64_t costBi;                 /* uiCostBi */
  uint32_t bits[3];                /* uiBits */
  int32_t  refIdx[2];              /* iRefIdx */
  int32_t  mv[2][2];               /* cMv */
  int32_t  refIdxBi[2];            /* iRefIdxBi */
  int32_t  mvBi[2][2];             /* cMvBi */
  int32_t  refineList;             /* the list the bi stage searched */
  int32_t  interDir;               /* pu.interDir: 1 list 0, 2 list 1, 3 bi-prediction */
  int32_t  smvdMode;               /* symMode (:2789): 1 when the symmetric-MVD pair replaced the bi vectors, else 0 */
  int32_t  mvpIdxL1Zero;           /* MvdL1Zero pictures: bestBiPMvpL1 (:2382-2387), the list-1 predictor index of the bi mode (its vector IS the predictor: mvBi[1], refIdxBi[1]) */
  int32_t  pad;
} vtmhip_pis_pu;

/* per-PU state of the CU recursion that predInterSearch reads */
typedef struct
{
  uint8_t  noSmvd;                 /* !trySmvd (:2301) */
  uint8_t  uniMvInsert;            /* insertUniMvCands runs between the uni loop and the bi stage (:2451-2459: cu.imv == 0, default BCW): the bi searches and the SMVD
                                      start list see the PU's own uni vectors in m_uniMvList */
  uint8_t  uniMvSelfIsNew;         /* with uniMvInsert: the block has no entry yet -- its vectors become the newest entry (of 15 entries the oldest drops out) */
  int8_t   bcwWeightL1;            /* g_BcwWeights[cu.BcwIdx] = getBcwWeight( cu.BcwIdx, REF_PIC_LIST_1 ) in {-2, 3, 4, 5, 10}; 0 or 4: the default weight.  Another weight (list 0 then
                                      weighs 8 - w): the bi stage refines the list with the SMALLER |weight| (:2556-2559) against the weighted target, prices with |w| / 8, skips the refined
                                      list's pictures that have the other list's POC (bcwFastSkipPoc, :2588-2593) and ENFORCES the bi mode (enforceBcwPred :2543, 2843-2847) */
  int16_t  uniMvSelfPos;           /* with uniMvInsert && !uniMvSelfIsNew: position (newest first, 0 .. 14) of the block's entry, overwritten in place (InterSearch.h:247-275) */
  uint8_t  bcwIdxBits;             /* getWeightIdxBits( cu.BcwIdx ) when sps.getUseBcw(), else 0: joins every bi row's bits and the SMVD mode bits (:2595, 2781) */
  uint8_t  bcwFastSkipPoc;         /* m_pcEncCfg->getUseBcwFast() && slice.getTLayer() > 1 (the device adds: weight != default && cu.imv == 0) */
} vtmhip_pis_pu_in;                /* 8 bytes as in ABI 5 (uniMvSelfPos was an int32 holding 0 .. 14: records of ABI 5 read unchanged, with the BCW fields 0) */

typedef struct
{
  int32_t  numPU;
  int32_t  numRef[2];              /* slice.getNumRefIdx(); numRef[1] == 0: P slice */
  int32_t  smvdBit;                /* slice.getBiDirPred(): one more bit on the bi rows (:2590-2593) */
  uint32_t mbBits[3];              /* xGetBlkBits (:3164-3169) */
  int32_t  refStride;
  int64_t  refPlaneOff[2][VTMHIP_MAX_REF];   /* sample offset of each reference plane's (0,0) inside d_refBase */
  vtmhip_me_job        *uniJobs;   /* [(numRef[0] + numRef[1]) * numPU]: static fields by the host, candidates / bits by stage 0 */
  const vtmhip_me_out  *uniOut;
  vtmhip_pis_row       *uniRows;
  vtmhip_pis_pu        *pus;       /* [numPU] */
  vtmhip_pred_job      *predOther; /* [numPU]: static fields by the host; mode / refOff / mv by stage 2 */
  vtmhip_me_job        *biJobs;    /* [numRef[refined list] * numPU] (numRef[0] == numRef[1] in B slices here) */
  const vtmhip_me_out  *biOut;
  vtmhip_pred_job      *predFinal; /* [numPU] */
  const int32_t        *parentIdx; /* [numPU] PU index in the parent level, or -1 (NULL: no parent level) */
  const vtmhip_pis_row *parentRows;/* the parent level's uniRows */
  int32_t  parentNumPU, pad;
  const int64_t        *pos;       /* [numPU] y * refStride + x */
  /* final prediction of the chosen mode (InterPrediction::motionCompensation with luma and chroma): BDOF where xPredInterBi applies it (:527-572) and
   * the two 4:2:0 chroma planes */
  int32_t  bdofEnabled;            /* sps.getBDOFEnabledFlag() && !picHeader.getDisBdofFlag() */
  int32_t  curPoc;
  int32_t  refPoc[2][VTMHIP_MAX_REF];
  vtmhip_pred_job      *predFinalC;/* [2 * numPU] or NULL: the Cb jobs, then the Cr jobs (static fields by the host; mode / refOff / mv by the final stage) */
  const int64_t        *posC;      /* [numPU] (y / 2) * refStrideC + x / 2 */
  int64_t  refPlaneOffC[2][2][VTMHIP_MAX_REF];   /* [Cb / Cr][list][refIdx] sample offset of the chroma plane's (0,0) inside d_refBase */
  /* affine uni stage (predAffineInterSearch's uni loop :4480-4660, 4-parameter model) for PUs of at least 16x16: one xAffineMotionEstimation job per
   * (PU, list, refIdx) row, starting from / predicted by the row's translational result (the affine AMVP list needs the CU recursion: stand-in as for AMVP) */
  vtmhip_affine_me_job *affJobs;   /* [(numRef[0] + numRef[1]) * numPU] or NULL; filled by stage 4 */
  int32_t  affLowDelay;            /* m_pcEncCfg->getIntraPeriod() == -1 (refinement rounds) */
  int32_t  affCheckLDC;            /* slice.getCheckLDC(): PROF's large-gradient rule */
  /* SMVD block (:2656-2790) between the bi refinement and the uni / bi decision, when the slice has a symmetric reference pair (smvdBit != 0): one
   * vtmhip_smvd_job per PU, searched list = list 0 */
  vtmhip_smvd_job      *smvdJobs;  /* [numPU] or NULL; filled by stage 3, searched by vtmhip_smvd_batch_dev( VTMHIP_SMVD_SEARCH ), merged by stage 5 */
  int32_t  symRefIdx[2];           /* slice.getSymRefIdx( list ) */
  /* ---- the caller's CU context instead of the level-order stand-ins (vtmhip_predInterSearch_batch_dev: one call = predInterSearch of n real PUs) ---- */
  int32_t  candsGiven;             /* != 0: uniJobs already hold the real AMVP lists (PU::fillMvpCand: amvpCand, numAmvpCand 1 or 2), mvpIdxBits, the m_uniMvList start vectors
                                      (numExtraStart / extraStart), imv, flags and the entry bits (mbBits + reference-index bits): stage 0 is skipped */
  int32_t  biRestricted;           /* PU::isBipredRestriction (8x4 / 4x8): no bi stage, no SMVD */
  int32_t  list1FromList0[VTMHIP_MAX_REF]; /* slice.getList1IdxToList0Idx( refIdx ) + 1: v > 0: list-1 picture refIdx is list-0 picture v - 1.  Such a row never becomes the uni-directional
                                      list-1 result (mvValidList1 / costValidList1, :2438-2446, 2826-2829); with fastMEForGenBLowDelay it is not searched either.  0: a picture of its own */
  const vtmhip_pis_pu_in *puIn;    /* [numPU] or NULL */
  vtmhip_pis_row       *biRows;    /* [numRef[refined list] * numPU] or NULL: the bi rows after xCheckBestMVP (cMvTemp, cMvPredBi, aaiMvpIdxBi, bits, cost) */
  uint64_t             *distBiP;   /* [(numRef[0] + numRef[1]) * numPU] or NULL: *puiDistBiP of xEstimateMvPredAMVP per row */
  int32_t  mvdL1Zero;              /* picHeader.getMvdL1ZeroFlag() (both lists hold the same pictures): the bi mode takes list 1 AT its best AMVP predictor (smallest template cost over
                                      the list-1 rows, :2382-2387, 2477-2522: needs distBiP) and refines list 0 only (:2576-2580) */
  int32_t  fastMEForGenBLowDelay;  /* cfg FDM (:2391-2404): the rows of list-1 pictures that are list-0 pictures too take the list-0 vector and a re-priced cost instead of a search */
  int32_t  givenRows;              /* bit ( list ? numRef[0] : 0 ) + refIdx: every row of that (list, refIdx) carries VTMHIP_MEJ_GIVEN_UNI -- the group is not searched */
  int32_t  picW, picH, ctuSize;    /* picW != 0: the other list's vector is clipped as motionCompensation does it (clipMv, InterPrediction.cpp:445-470) before the prediction for the bi
                                      refinement is formed -- search results are inside the clip range by construction, an AMVP predictor (MvdL1Zero) need not be */
} vtmhip_pis_level;


/* stage 0: AMVP candidates and entry bits of the uni rows (before vtmhip_xEstimateMvPredAMVP_batch_dev)
 * stage 1: after the uni searches: xCheckBestMVP per row, best reference per list; P slices: interDir and predFinal
 * stage 2: B slices: refined list, predOther (the other list's prediction, epilogue as the host set it), the bi rows
 * stage 3: after the bi searches: xCheckBestMVP, best bi row, decision, predFinal; with smvdJobs: the SMVD job of every PU instead of the decision (start
 *          vectors cMvHevcTemp / cMvTemp / cMvBi of list 0's symmetric reference; the m_uniMvList history is CU-recursion state and stays empty)
 * stage 5: (smvdJobs != NULL) after the SMVD search: symCost < uiCostBi replaces the bi vectors (:2787-2803), then the decision and predFinal (no BDOF for an
 *          SMVD pair, InterPrediction.cpp:552-555)
 * stage 4: (affJobs != NULL) the affine uni jobs of every row: start vector and predictor = the row's translational result at all control points,
 *          bits = the row's bits before the vector rate, hevcCost = the PU's best translational cost -> vtmhip_xAffineMotionEstimation_batch_dev */
int vtmhip_pis_stage( vtmhip_ctx *ctx, const vtmhip_pis_level *lvl, int stage );

/* ---- the level-order picture loop itself, natively -------------------------------------------------------------------------------------------
 * One call runs the whole chain of a picture over the levels' tables (what vtm_amd/pipeline.py:FrameHotPath.run does call by call from Python:
 * ~130 library calls, 2 ms of interpreter time per picture -- more than a GPU needs for its share of a picture sharded over eight GPUs).
 * Per level: stage 0, xEstimateMvPredAMVP, the uni searches, stage 1 on `mainStream` (a level's AMVP candidates are its parent's vectors: one dependent
 * chain); everything after that -- stage 2, the other list's prediction, the bi refinement, stage 3, (the SMVD search, stage 5,) the final prediction (plain / BDOF / chroma),
 * the affine uni stage, the TU chains -- on sideStreams[level % numSide] behind an event, beside the next levels' searches; the side streams join
 * `mainStream` at the end.  numSide == 0: everything on mainStream in level order.  The context's stream is mainStream on return. */
typedef struct
{
  vtmhip_pis_level  pis;
  vtmhip_pic_params pic, picBi;        /* wavesPerJob tuned per level for the uni / bi searches */
  vtmhip_me_cfg     cfgUni, cfgBi;
  int32_t  width, height;              /* the level's PU shape */
  int32_t  bdof;                       /* launch vtmhip_bdof_batch_dev over predFinal after the plain prediction */
  int32_t  pad0;
  vtmhip_me_out        *uniOut;        /* = pis.uniOut, writable */
  vtmhip_me_out        *biOut;
  /* luma TU chains: `numCands` candidate runs of `numTU` jobs each, stored one after the other in tu[] / tuRes[]; cand[i] = 1: transform skip */
  vtmhip_tu_job        *tu;
  vtmhip_tu_result     *tuRes;
  int32_t              *qcoef;
  int32_t  numTU, numCands, tuW, tuH;
  uint8_t  cand[8];
  /* chroma TU chains (NULL: none): 2 * numTUC jobs (Cb then Cr) */
  vtmhip_tu_job        *tuC;
  vtmhip_tu_result     *tuResC;
  int32_t              *qcoefC;
  int32_t  numTUC, tuWC, tuHC, pad1;
  vtmhip_affine_me_out *affOut;        /* affine uni stage when pis.affJobs != NULL */
  uint8_t *mtsTest;                    /* [numCands * numTU] or NULL: the MTS pre-selection flags of the luma candidates (vtmhip_mts_select_batch_dev) */
  int32_t  mtsMaxCand, pad2;           /* cfg MTSInterMaxCand */
} vtmhip_pis_level_run;

typedef struct
{
  const int16_t *org;                  /* original picture (Y | Cb | Cr) */
  const int16_t *dpb;                  /* reference pictures */
  int16_t *pred, *resi;                /* level-wide luma sample buffers (compact per-PU slots, offsets in the job tables) */
  int16_t *orgBi;                      /* 2 * org - pred of the other list (B slices) */
  int16_t *predC, *resiC;              /* chroma (NULL: luma only) */
} vtmhip_pis_buffers;

int vtmhip_pis_run_picture( vtmhip_ctx *ctx, const vtmhip_pis_level_run *levels, int numLevels, const vtmhip_pis_buffers *buf, void *mainStream,
                            void *const *sideStreams, int numSide );

/* ---- InterSearch::predInterSearch (InterSearch.cpp:2245-2893, the translational part incl. the SMVD block) of n real PUs of one slice and one block shape in ONE call ------
 * The batched hook a CU-level integration uses (oracle/ref_shim_enc.cpp drives it from inside the real encoder): L->pis.candsGiven = 1, the
 * uni rows carry the PUs' real AMVP lists, m_uniMvList start vectors, cu.imv (0 .. 3: fractional or AMVR integer refinement) and block-vector cache hits.  Runs on the
 * context's stream, no host synchronisation:
 *   xEstimateMvPredAMVP per row -> xMotionEstimation per searched row -> xCheckBestMVP, list-1 rows copied from list 0 (FastMEForGenBLowDelay), best reference per list
 *   -> B slices without bi-prediction restriction: the other list's prediction, the bi refinement of the costlier list (one iteration: FASTINTERSEARCH_MODE1 / 2), xCheckBestMVP
 *   -> the SMVD block (L->pis.smvdJobs) -> uni / bi decision.
 * Results: L->pis.uniRows, L->uniOut (every row's vector / bits / cost BEFORE xCheckBestMVP: what m_uniMotions and the block-vector cache store), L->pis.biRows, L->biOut,
 * L->pis.smvdJobs (with the trace), L->pis.pus.  No prediction, no residual coding (predFinal may be NULL); buf->orgBi: numPU * width * height samples of scratch.
 * Covered: P and B slices, cu.imv 0 .. 3, block-vector cache hits, m_uniMvList, FastMEForGenBLowDelay copies, MvdL1Zero pictures (mvdL1Zero, distBiP, mvpIdxL1Zero),
 * bi-prediction restriction, the SMVD block, BCW (ABI 6): the weight-index bits (puIn.bcwIdxBits) and CU-level weights other than the default (puIn.bcwWeightL1, given uni rows).
 * Not covered (the caller keeps the reference path): explicit weighted prediction, four bi iterations (FEN off), MCTS, composite references, hash ME, IBC.
 * Synchronisation: none for the shapes vtmhip_is_uniform_shape() accepts and for every call with fewer than 64 rows (a CU-level hook); a batch of >= 64 rows of another shape
 * (64x8, 128x64, ...) is bucketed by shape inside vtmhip_xMotionEstimation_batch_dev, which synchronises the stream once to read the class counts (never under stream capture). */
int vtmhip_predInterSearch_batch_dev( vtmhip_ctx *ctx, const vtmhip_pis_level_run *L, const vtmhip_pis_buffers *buf );
/* 1 when a batch of width x height blocks may promise cfg.uniformSquare (the tiled kernels know the shape) */
int vtmhip_is_uniform_shape( int width, int height );
/* Row-band form of the integer search kernel (tz_search_kernel: a thread keeps K segments of the block for the whole search, a round loads all its candidates at once): the K
 * (1, 2 or 4) a fused uniform launch of width x height blocks at this row sub-sampling shift and pic.wavesPerJob runs with, 0 when the launch keeps the by-candidate kernel
 * (4-sample segments, widths 12 / 24 / 48, a block that K * 64 * wavesPerJob threads do not cover exactly).  Job-table calls (vtmhip_tz_search_batch_dev) always keep that
 * kernel; so does every launch when VTMHIP_TZ_BANDS=0 is set in the environment. */
int vtmhip_tz_band_items( int width, int height, int subShift, int wavesPerJob );

/* ---- raster pruning: 8x8 box sums of the reference planes ---------------------------------------------------------------------------------------------
 * The raster scan of xTZSearch (split search: tz_raster_cols_kernel) skips grid points that a block-sum lower bound rules out: over the 8x8 sub-blocks of the block,
 * sum |sum(org sub-block) - sum(ref sub-block)| <= SAD, and a point whose bound + MV rate is not below the best cost the search holds when the scan starts can never be
 * accepted.  A scan without such a point is skipped; otherwise the bounding rectangle of the remaining points is scanned.  Results do not change.
 * The bound reads a SUM BUFFER congruent with the reference planes: d_sumBase[off] is the sum of the 8x8 samples whose first is d_refBase[off].
 *   vtmhip_tz_box_sums_dev: the sums of ONE luma plane (its sample (0,0) at d_refBase + planeOff, `margin` >= ctuSize + 16 border samples on every side, as the planes of
 *     every *_dev call carry), on the context's stream.  Written: x in [-(margin - 9), width + margin - 17], y in [-(margin - 9), height + margin - 17] -- every position
 *     clipMv leaves to a block origin (-(ctuSize + 7) .. size + 7 with ctuSize = margin - 16) and the block's further sub-blocks; read: samples up to size + margin - 10,
 *     nothing outside the plane's border.  Samples are unsigned and at most 10 bits deep (64 * 1023 fits 16 bits).
 *   vtmhip_tz_attach_sums: from now on the TZ searches of this context whose d_refBase is `d_refBase` use d_sumBase (d_sumBase NULL: detach).  One buffer at a time.
 *     width / height / margin: what the sums were computed with (every plane alike).  A search uses them only when its vtmhip_pic_params name the same picture size and
 *     margin >= ctuSize + 16, i.e. when the sums cover every position its scan can take; any other search runs the full scan.
 *     CONTRACT: attached sums describe the CURRENT contents of every plane the searches read, computed for the picture size the searches pass in vtmhip_pic_params; the
 *     caller recomputes them (stream-ordered before the search) whenever a plane changes.  With nothing attached nothing changes.  Jobs the bound does not apply to
 *     (subShift != 0, signedSamples, bitDepth > 10, a width or height that is no multiple of 8, the in-kernel scans) run the full scan.
 *     vtmhip_pis_run_picture computes and attaches the sums of the picture's reference planes itself and, on return, puts back whatever the caller had attached
 *     (a picture the bound does not apply to -- bitDepth > 10, no level with subShift 0, levels of different geometry -- runs with the caller's attachment untouched).
 *     Its sum buffer is a workspace of the context, about the size of the DPB span of the referenced planes, kept per main stream.  FIRST-CALL CONTRACT, as for the
 *     other per-stream workspaces: the first picture of a geometry on a main stream (and any later picture that needs a larger span) allocates it -- a stream
 *     synchronise, a hipFree of the smaller block (which waits for the device, the side stream's pass included) and a hipMalloc -- so run one picture eagerly on a
 *     stream before timing it or capturing it into a graph (bench.py --graph does exactly that).  The block is written on the first side stream and read by the
 *     raster launches on the main stream, ordered by events inside the call.
 *   vtmhip_tz_prune_stats: stats[6] = raster scans listed for the column kernel, scans skipped, scans reduced to a proper sub-rectangle, grid points evaluated, grid
 *     points of all listed scans, scans whose winner was below the best cost on entry (the search accepts it) -- of this context since the last reset (stats may be NULL; reset != 0 clears).  Synchronises the context's stream.
 * ROUND BOUND: the same sums rule out candidates of the diamond, star and two-point rounds in the fused uniform launches of 128x128 and 128x64 rows at
 * wavesPerJob 8 (subShift 0, bitDepth <= 10, unsigned samples): a round first forms each candidate's bound (512 B against the 32 KB of its samples) and evaluates only
 * the candidates whose bound + MV rate is below the best cost the search holds.  Results, nEval and vtmhip_tz_prune_stats do not change.
 *   vtmhip_tz_round_stats: stats[7] = rounds bounded, candidates listed in them, candidates skipped of the first launches (modes 0 / 1), the same three of the resume
 *     launches (mode 2), and `violations`: evaluated candidates whose exact SAD came out below their bound -- the kernel's own check that sums and planes are
 *     congruent, 0 unless the CONTRACT above is broken.  Of this context since the last reset (stats may be NULL; reset != 0 clears).  Synchronises the context's stream.
 * VTMHIP_TZ_PRUNE=0 in the environment: the sums are ignored (and the picture loop computes none).  VTMHIP_TZ_ROUND_BOUND=0: the list rounds ignore them. */
int vtmhip_tz_box_sums_dev( vtmhip_ctx *ctx, const int16_t *d_refBase, uint16_t *d_sumBase, int64_t planeOff, int stride, int width, int height, int margin );
int vtmhip_tz_attach_sums( vtmhip_ctx *ctx, const int16_t *d_refBase, const uint16_t *d_sumBase, int width, int height, int margin );
int vtmhip_tz_prune_stats( vtmhip_ctx *ctx, uint64_t *stats, int reset );
int vtmhip_tz_round_stats( vtmhip_ctx *ctx, uint64_t *stats, int reset );

/* ---- sub-block transform (SBT) of inter CUs: the mode estimator and the SBT candidates of xEstimateInterResidualQT --------------------------------
 * (CodingUnit::checkAllowedSbt Unit.cpp:450-494; CU::getSbtMode ... numSbtModeRdo UnitTools.cpp:3516-3589; PartitionerImpl::getSbtTuTiling
 * UnitPartitioner.cpp:1091-1148; TrQuant::getTrTypes TrQuant.cpp:728-760; InterSearch::calcMinDistSbt / skipSbtByRDCost InterSearch.cpp:6195-6438.)
 * The rules have one definition for host and device, vtm_amd/csrc/sbt_rules.hpp:
 *   sbtIdx 1 VER_HALF, 2 HOR_HALF, 3 VER_QUAD, 4 HOR_QUAD; sbtPos 0 / 1; sbtMode = (sbtIdx - 1) * 2 + sbtPos (0 .. 7); sbtAllowed: bit sbtIdx set.
 *   Allowed by size: both sides <= maxTbSize, VER_HALF w >= 8, HOR_HALF h >= 8, VER_QUAD w >= 16, HOR_QUAD h >= 16 (prediction mode and CIIP: the caller's).
 *   Coded tile of a component block cw x ch: POS0 the first 1/2 (1/4) of the split side, POS1 the last; every factor is (dim * f) >> 2 on the component's block.
 *   Luma transform pair: vertical splits DCT2 / DCT2 when the sub-TU's height > 32, else POS0 (hor DCT8, ver DST7), POS1 (DST7, DST7); horizontal splits
 *   DCT2 / DCT2 when its width > 32, else POS0 (DST7, DCT8), POS1 (DST7, DST7).  Chroma: DCT2 / DCT2.  No transform skip, no MTS.
 * 4:2:0 only.  Out of scope: the level-order picture driver, JCCR or chroma residual scaling on SBT sub-TUs, the CABAC estimate, m_histBestSbt and the
 * save / load of SBT decisions, ACT. */
#define VTMHIP_SBT_VER_HALF 1
#define VTMHIP_SBT_HOR_HALF 2
#define VTMHIP_SBT_VER_QUAD 3
#define VTMHIP_SBT_HOR_QUAD 4

typedef struct
{
  int64_t orgOff[3], predOff[3];      /* the CU's original / prediction blocks of Y, Cb, Cr inside d_orgBase / d_predBase; a chroma offset of -1 (either one): luma only */
  int32_t orgStride[3], predStride[3];
  int16_t width, height;              /* the LUMA CU size, powers of two 4 .. 64; chroma blocks are width / 2 x height / 2 */
  uint8_t bitDepth;                   /* 8 .. 12 */
  uint8_t sbtAllowed;                 /* the CU's mask; a type the size rule above excludes makes the job invalid */
  uint8_t pad0, pad1;
  double  chromaWeight;               /* RdCost::getChromaWeight() */
  double  distScale;                  /* RdCost::m_DistScaleUnadjusted: calcRdCost( bits, dist ) = distScale * dist + bits */
} vtmhip_sbt_est_job;

typedef struct
{
  uint64_t est[9];                    /* m_estMinDistSbt: [sbtMode] (UINT64_MAX: not tried), [8] = the CU's SSE over the partitions */
  uint8_t  rdoOrder[8];               /* m_sbtRdoOrder, 255-filled */
  uint32_t part[3][4][4];             /* the raw partition sums [component][j][i] BEFORE the chroma weight (zero outside numPartY x numPartX and for absent chroma) */
  uint8_t  skipAll;                   /* m_skipSbtAll: distScale * est[8] < 12 << 15; est[0 .. 7] and rdoOrder then stay UINT64_MAX / 255 */
  uint8_t  pad[7];
} vtmhip_sbt_est_result;

/* InterSearch::calcMinDistSbt for n CUs, one launch.  numPartX / numPartY = 4 for a luma side >= 16, 1 for 4, 2 otherwise; every component's block is divided by
 * that count; a chroma partition sum becomes (uint64)( double( sum ) * chromaWeight ) before it joins dist[j][i].  Squared differences are added at full
 * precision: the reference's shift DISTORTION_PRECISION_ADJUSTMENT( ( bitDepth - 8 ) << 1 ) is 0 as it is built (FULL_NBIT = 1, TypeDef.h:228-233; sbtDistShift in
 * sbt_rules.hpp is the one place that says so).  Samples lie within the bit depth (|org - pred| <= 4095), so a partition sum -- at most 256 samples -- fits 32
 * bits (by 2 096 896 at 12 bits: a difference outside the bit depth wraps the sum silently; the caller's contract, as for every sample entry here).  maxWidth x maxHeight (the largest luma CU of the batch)
 * sizes the lanes a CU gets: 16 (up to 256 luma samples: four CUs share a wave), a wave (up to 1024) or a workgroup; a larger job is still computed.
 * The jobs stay on the device: a job with a side outside 4 .. 64 or not a power of two, a bitDepth outside 8 .. 12 or a sbtAllowed the size rule (maxTbSize 64)
 * excludes is skipped -- its result is not written.  A CU with sbtAllowed == 0 gets est[8] and part[] by the same partition rule (the reference takes
 * getDistPart there, which rounds the chroma weight differently: keep that case on the host if the value matters). */
int vtmhip_sbt_est_batch_dev( vtmhip_ctx *ctx, const int16_t *d_orgBase, const int16_t *d_predBase, const vtmhip_sbt_est_job *d_jobs, int n, int maxWidth,
                              int maxHeight, vtmhip_sbt_est_result *d_results );

/* InterSearch::skipSbtByRDCost over an est[9] record (host arithmetic, no device; the double operations in the reference's order): the early-skip type 0 .. 3,
 * or 255 to try the mode.  costSbtOff == MAX_DOUBLE (1.7e+308): no SBT-off result yet.  A NULL est or a mode outside the table returns VTMHIP_E_INVALID. */
int vtmhip_sbt_skip_by_rdcost( const uint64_t est[9], double distScale, int sbtIdx, int sbtPos, double bestCost, uint64_t distSbtOff, double costSbtOff,
                               int rootCbfSbtOff );

typedef struct
{
  int64_t resiOff[3];                 /* the CU's residual of Y, Cb, Cr inside d_resiBase; a chroma offset of -1: that component is not coded */
  int64_t outOff[3];                  /* per component: the sub-TU's levels (sub-W x sub-H contiguous) inside d_levelsBase and the CU-shaped reconstructed residual
                                         (comp-W x comp-H contiguous) inside d_recBase */
  int32_t resiStride[3];
  int16_t width, height;              /* the LUMA CU size, powers of two 4 .. 64 */
  int16_t qpPer[3], qpRem[3];         /* as vtmhip_tu_job, per component */
  uint8_t sbtIdx, sbtPos;             /* VTMHIP_SBT_*, 0 / 1 */
  uint8_t bitDepth, isIRAP;           /* bitDepth 8 .. 12 */
} vtmhip_sbt_job;

typedef struct
{
  uint64_t sseCoded[3];               /* the chain's SSE over the coded tile (vtmhip_tu_result.sse); unweighted: the caller applies the chroma distortion weight */
  uint64_t sseZero[3];                /* sum of r * r over the uncoded tile's residual (full precision, as sseCoded: see vtmhip_sbt_est_batch_dev) */
  int32_t  absSum[3];                 /* uiAbsSum of Quant::quant on the sub-TU */
  int32_t  pad;
} vtmhip_sbt_result;                  /* an absent component's fields are zero */

/* One (CU, sbtIdx, sbtPos) candidate per job, no host round trip between the steps: an expansion kernel turns every job into one vtmhip_tu_job per present
 * component (the sub-TU rectangle inside the CU's residual, the transform pair above), the fused chain runs them through the launch paths of
 * vtmhip_tu_chain_batch_dev with uniformSize == 0 (256 or more sub-TUs: bucketed by shape), and a finish kernel completes the candidate: sseCoded / absSum from
 * the chain, sseZero, and -- when d_recBase is given -- the CU-shaped reconstruction with the coded tile from the chain and zeros elsewhere.  d_levelsBase and
 * d_recBase may be NULL.  The chain writes the compact sub-TU reconstruction to the head of the CU-shaped block; the finish kernel spreads it in place, so the
 * only scratch is the expanded job table and its results (the context's workspace of the stream, no allocation once it has grown).
 * The job table is read back (n * 80 bytes, one stream synchronisation; never under stream capture) and checked before anything is launched: a side outside
 * 4 .. 64 or not a power of two, a mode the size rule (maxTbSize 64) does not allow, sbtPos > 1, a bitDepth outside 8 .. 12, qpRem outside 0 .. 5, qpPer < 0, a
 * negative luma offset or a NULL pointer return VTMHIP_E_INVALID and launch nothing.  n == 0 is VTMHIP_OK. */
int vtmhip_sbt_chain_batch_dev( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_sbt_job *d_jobs, int n, int32_t *d_levelsBase, int16_t *d_recBase,
                                vtmhip_sbt_result *d_results );

/* The same expansion as host arithmetic, for callers that keep their own job tables: out[i] = the luma sub-TU of job i (i < n), the chroma sub-TUs follow from
 * out[n] on in job order (Cb before Cr); tuIdx[3 * i + c] = the index of job i's component c inside out, -1 when absent (may be NULL).  out holds up to 3 * n
 * jobs; *numOut receives the count.  The checks of vtmhip_sbt_chain_batch_dev apply. */
int vtmhip_sbt_make_tu_jobs( const vtmhip_sbt_job *jobs, int n, vtmhip_tu_job *out, int *numOut, int32_t *tuIdx );

int vtmhip_sbt_struct_size( int which );   /* sizeof() of 0 vtmhip_sbt_est_job, 1 vtmhip_sbt_est_result, 2 vtmhip_sbt_job, 3 vtmhip_sbt_result; -1 otherwise */

/* ---- intra luma prediction: IntraPrediction::predIntraAng (CommonLib/IntraPrediction.cpp:217-266) for a luma block without ISP, MIP or BDPCM, and the first-round
 * mode pre-selection of IntraSearch::estIntraPredLumaQT (EncoderLib/IntraSearch.cpp:549-700) fused on top of it.  The rules have one definition for host and
 * device, vtm_amd/csrc/intra_rules.hpp:
 *   parameters        initPredIntraParams :356-444 with getModifiedWideAngle :184-204 and the MDIS thresholds m_aucIntraFilter :58-68
 *   filtered lines    xFilterReferenceSamples :1166-1200, computed on the device from the unfiltered ones
 *   planar, DC        xPredIntraPlanar :294-348, xGetPredValDc :153-182, their PDPC :244-265
 *   angular           xPredIntraAng :459-643: pure horizontal / vertical with the clipped PDPC, the extension of the main reference through invAngle for negative
 *                     angles, the replication of its last sample for positive ones, the cubic (H.266 table 28) or smoothing taps on fractional slopes, the PDPC column
 * BDPCM, IntraSmoothingDisabled, the availability analysis that fills the reference samples (xFillReferenceSamples), the mode bits and the
 * candidate lists stay the caller's.  Chroma, MIP and ISP have entries of their own below (vtmhip_intra_chroma_*, vtmhip_mip_*, vtmhip_isp_*). */
typedef struct
{
  int32_t predMode;            /* the mode after the wide-angle shift: -14 .. 80 (what the angle is taken from) */
  int32_t isModeVer;
  int32_t intraPredAngle;
  int32_t invAngle;
  int32_t angularScale;        /* set for positive angles, 0 otherwise (the reference leaves it untouched there) */
  int32_t applyPDPC;
  int32_t refFilterFlag;       /* predict from the [1 2 1]-filtered lines */
  int32_t interpolationFlag;   /* fractional slopes take the smoothing taps instead of the cubic ones */
} vtmhip_intra_params;

/* m_ipaParam of a width x height luma block (sides 4, 8, 16, 32, 64), mode 0 .. 66, multiRefIdx 0 .. 2 (not 0 with planar): host arithmetic, no context.
 * Anything else returns VTMHIP_E_INVALID. */
int vtmhip_intra_pred_params( int width, int height, int mode, int multiRefIdx, vtmhip_intra_params *out );

typedef struct
{
  int64_t refOff;      /* top line: d_refBase[refOff .. refOff + 2W + m], index 0 = the corner sample of line m;
                          the left line follows directly: 2H + 1 + m samples, index 0 = the same corner
                          (the reference's unfiltered buffer with predStride = 2W + 1 + m) */
  int64_t orgOff;      /* original block inside d_orgBase (the pre-selection entries and vtmhip_intra_chain_batch_dev) */
  int32_t orgStride;
  int16_t width, height;   /* 4, 8, 16, 32, 64 each; every combination */
  uint8_t bitDepth;        /* 8 .. 12; clip range [0, (1 << bitDepth) - 1] */
  uint8_t multiRefIdx;     /* 0, 1, 2 (MULTI_REF_LINE_IDX) */
  uint8_t reserved[2];     /* 0 */
} vtmhip_intra_block;

typedef struct
{
  int64_t predOff;     /* vtmhip_intra_pred_batch_dev and vtmhip_intra_chain_batch_dev: the W x H prediction (stride W) inside d_predBase; the latter writes the
                          residual at the same offset inside d_resiBase */
  int32_t block;       /* index into d_blocks */
  uint8_t mode;        /* 0 planar, 1 DC, 2 .. 66 */
  uint8_t reserved[3]; /* 0 */
} vtmhip_intra_job;

/* predIntraAng, PDPC included, for n (block, mode) jobs: job k writes width x height samples with stride width at d_predBase + predOff.  Only the job's own lines
 * are read: 2W + 1 + m and 2H + 1 + m samples from refOff on; where the reference replicates the last sample of the main line, the device repeats the index.
 * Jobs of one block that follow each other in d_jobs share one load of its lines (and of its original block below); any order is allowed.
 * NULL pointers, n < 0, numBlocks < 0 and numBlocks == 0 with n > 0 return VTMHIP_E_INVALID; n == 0 is VTMHIP_OK.  The tables stay on the device: a job whose
 * block index is outside [0, numBlocks), whose mode is above 66 or planar with multiRefIdx != 0, or whose block has a side outside the list, a bitDepth outside
 * 8 .. 12 or a multiRefIdx above 2 is skipped -- nothing is read through it and its output is not written (as vtmhip_sbt_est_batch_dev skips its invalid jobs).
 * The largest well-formed block of d_blocks decides how many lanes a job gets (vtmhip_intra_lanes_per_job); a small kernel finds it, so there is no read-back. */
int vtmhip_intra_pred_batch_dev( vtmhip_ctx *ctx, const int16_t *d_refBase, const vtmhip_intra_block *d_blocks, int numBlocks, const vtmhip_intra_job *d_jobs, int n,
                                 int16_t *d_predBase );

/* The same prediction formed in LDS and consumed there: d_dist[2 k] = the SAD of job k's prediction against its block's original, d_dist[2 k + 1] = the SATD under
 * the xGetHADs tile rules (the DistParam::distFunc slots of IntraSearch.cpp:573-592).  No sample of a prediction goes to global memory; predOff is ignored.
 * min( 2 * SAD, SATD ), the mode bits and the candidate lists stay the caller's.  Checks and skipped jobs as above (both d_dist entries of a skipped job are left). */
int vtmhip_intra_presel_batch_dev( vtmhip_ctx *ctx, const int16_t *d_refBase, const int16_t *d_orgBase, const vtmhip_intra_block *d_blocks, int numBlocks,
                                   const vtmhip_intra_job *d_jobs, int n, uint64_t *d_dist );

/* lanes a job gets when the largest block of the table has maxArea = width * height samples: 16 (up to 64 samples: sixteen jobs per workgroup at once), 64 (up to
 * 1024: a wave per job) or 256 (the workgroup per job); 0 for an area outside 16 .. 4096 */
int vtmhip_intra_lanes_per_job( int maxArea );

int vtmhip_intra_struct_size( int which );   /* sizeof() of 0 vtmhip_intra_params, 1 vtmhip_intra_block, 2 vtmhip_intra_job; -1 otherwise */

/* ---- intra chroma prediction for 4:2:0, Cb and Cr together, without BDPCM: the regular modes of a chroma block and the cross-component linear model
 * (LM 67, MDLM_L 68, MDLM_T 69; CommonDef.h:256-260), and the mode pre-selection of IntraSearch::estIntraPredChromaQT (EncoderLib/IntraSearch.cpp:1308-1414)
 * fused on top of them.  One definition for host and device, vtm_amd/csrc/cclm_rules.hpp and intra_rules.hpp:
 *   regular modes     predIntraAng with !isLuma: no reference filter, no smoothing taps, the two-tap rule on fractional slopes (IntraPrediction.cpp:592-604); wide
 *                     angles, PDPC and DC from the chroma block's own width and height.  The mode is the final one (DM resolved by the caller).
 *   down-sampling     xGetLumaRecPixels :1324-1579: the 6-tap default, the 5-tap cross (sps_cclm_colocated_chroma_flag), the one-row 3-tap of the top neighbour
 *                     row in the first row of a CTU, leftPadding / abovePadding, the left column from luma columns -3 .. -1
 *   model             xGetLMParameters :1580-1795: template lengths, the four picked pairs, the min / max grouping, the division by the significand table
 *   prediction        clip( ( ( a * ds ) >> shift ) + b ), predIntraChromaLM :268-288
 * The availability analysis stays the caller's: it hands over the flags and counts below with the unfiltered Cb and Cr reference lines (as for luma, multiRefIdx 0)
 * and the luma reconstruction.  Chroma sides are 4, 8, 16 and 32; a side of 2 (the chroma of a 4-wide or 4-high luma CU) is NOT covered and such a block is
 * skipped as malformed.  BDPCM, 4:2:2 / 4:4:4, the mode bits and the candidate lists stay the caller's. */
typedef struct
{
  int64_t cbRefOff, crRefOff;   /* the component's top line d_refBase[off .. off + 2W], index 0 = the corner; its left line follows directly: 2H + 1 samples */
  int64_t cbOrgOff, crOrgOff;   /* original blocks inside d_orgBase (pre-selection and the chain, vtmhip_intra_chroma_chain_batch_dev) */
  int64_t lumaOff;              /* inside d_lumaBase: the luma reconstruction sample under chroma (0, 0).  Read around it (LM modes only): columns 0 .. 2W - 1 of
                                   rows 0 .. 2H - 1; with above, rows -3 .. -1 of columns (left ? -3 : 0) .. 2 (W + aboveRight) - 1; with left, columns -3 .. -1 of
                                   rows (above ? -3 : 0) .. 2 (H + belowLeft) - 1 */
  int32_t orgStride, lumaStride;
  int16_t width, height;            /* 4, 8, 16, 32 each; every combination */
  int16_t aboveRight, belowLeft;    /* available chroma samples beyond the block: multiples of 2, at most width / height, 0 without above / left */
  uint8_t bitDepth;                 /* 8 .. 12 */
  uint8_t above, left;              /* 0 / 1: the whole above row / left column of the block is available */
  uint8_t firstRow;                 /* 0 / 1: the block lies in the first luma row of its CTU */
  uint8_t colocated;                /* 0 / 1: sps_cclm_colocated_chroma_flag */
  uint8_t reserved[3];              /* 0 */
} vtmhip_intra_chroma_block;

typedef struct
{
  int64_t cbPredOff, crPredOff;   /* vtmhip_intra_chroma_pred_batch_dev and vtmhip_intra_chroma_chain_batch_dev: the W x H predictions (stride W) inside d_predBase;
                                     the latter writes the residuals at the same offsets inside d_resiBase */
  int32_t block;                  /* index into d_blocks */
  uint8_t mode;                   /* 0 .. 66 regular, 67 LM, 68 MDLM_L, 69 MDLM_T */
  uint8_t reserved[3];            /* 0 */
} vtmhip_intra_chroma_job;

typedef struct
{
  int32_t a, b, shift;
} vtmhip_cclm_model;

/* xGetLMParameters of one (block, component 0 Cb / 1 Cr, mode 67 .. 69): host arithmetic on host pointers, no context -- the block's offsets index refBase and
 * lumaBase as they index the device buffers below.  A malformed block, another mode or component, or a NULL pointer returns VTMHIP_E_INVALID. */
int vtmhip_cclm_params( const vtmhip_intra_chroma_block *block, const int16_t *refBase, const int16_t *lumaBase, int component, int mode, vtmhip_cclm_model *out );

/* The Cb and Cr predictions of n (block, mode) jobs: job k writes width x height samples with stride width at d_predBase + cbPredOff and + crPredOff.  Jobs of
 * one block that follow each other in d_jobs share one load of its lines and -- when one of them is an LM mode -- one down-sampling of its luma block; any order
 * is allowed.  d_lumaBase is read only through blocks that an LM job names.
 * NULL pointers, n < 0, numBlocks < 0 and numBlocks == 0 with n > 0 return VTMHIP_E_INVALID; n == 0 is VTMHIP_OK.  The tables stay on the device: a job whose
 * block index is outside [0, numBlocks) or whose mode is above 69, and every job of a block with a side outside 4 / 8 / 16 / 32, a bitDepth outside 8 .. 12, a
 * flag above 1 or inconsistent availability (aboveRight without above, belowLeft without left, a count that is odd, negative or beyond the side) is skipped --
 * nothing is read through it and its output is not written.  The largest well-formed block decides how many lanes a job gets (vtmhip_intra_lanes_per_job: 16 or
 * 64 here); a small kernel finds it, so there is no read-back. */
int vtmhip_intra_chroma_pred_batch_dev( vtmhip_ctx *ctx, const int16_t *d_refBase, const int16_t *d_lumaBase, const vtmhip_intra_chroma_block *d_blocks, int numBlocks,
                                        const vtmhip_intra_chroma_job *d_jobs, int n, int16_t *d_predBase );

/* The same predictions formed in LDS and consumed there: d_dist[4 k + 0 .. 3] = SAD Cb, SATD Cb, SAD Cr, SATD Cr of job k against its block's originals, the SATD
 * under the xGetHADs tile rules.  No sample of a prediction goes to global memory; the prediction offsets are ignored.  min( 2 * SAD, SATD ) per component, their
 * sum, the sort and the mode bits stay the caller's.  Checks and skipped jobs as above (all four entries of a skipped job are left). */
int vtmhip_intra_chroma_presel_batch_dev( vtmhip_ctx *ctx, const int16_t *d_refBase, const int16_t *d_lumaBase, const int16_t *d_orgBase,
                                          const vtmhip_intra_chroma_block *d_blocks, int numBlocks, const vtmhip_intra_chroma_job *d_jobs, int n, uint64_t *d_dist );

int vtmhip_intra_chroma_struct_size( int which );   /* sizeof() of 0 vtmhip_intra_chroma_block, 1 vtmhip_intra_chroma_job, 2 vtmhip_cclm_model; -1 otherwise */

/* ---- matrix-based intra prediction (MIP) of a luma block: MatrixIntraPrediction::prepareInputForPred / predBlock (CommonLib/MatrixIntraPrediction.cpp:62-137) and
 * the MIP candidates of IntraSearch::estIntraPredLumaQT (EncoderLib/IntraSearch.cpp:749-793: one initIntraMip per block, then predIntraMip and min( 2 * SAD, SATD )
 * for 2 * getNumModesMip (mode, transposed) pairs) fused on top of it.  One definition for host and device, vtm_amd/csrc/mip_rules.hpp:
 *   shape             getMipSizeId / getNumModesMip UnitTools.cpp:3873-3900 (4x4: 16 modes; a side of 4 or 8x8: 8; everything else: 6), initPredBlockParams :140-159
 *   reduced boundary  boundaryDownsampling1D :163-191 on top[1 .. W] and left[1 .. H], the two input orders and the rebasing of :94-117
 *   reduced block     computeReducedPred :283-335 with the caller's trained matrices (vtmhip_mip_set_tables), the clip and the transposition
 *   up-sampling       predictionUpsampling :194-267 as a closed form per sample (horizontal pass on the anchor rows, then vertical, each rounded)
 * Blocks are vtmhip_intra_block records with multiRefIdx 0, so one block table (and one pair of reference lines per block) serves the regular modes and MIP; of the
 * lines only top[1 .. W] and left[1 .. H] are read.  Every width x height of 4, 8, 16, 32, 64 is accepted.  MIP for chroma (4:4:4), the mode bits and the
 * candidate lists stay the caller's. */
typedef struct
{
  int64_t predOff;     /* vtmhip_mip_pred_batch_dev and vtmhip_intra_chain_batch_dev: the W x H prediction (stride W) inside d_predBase; the latter writes the
                          residual at the same offset inside d_resiBase */
  int32_t block;       /* index into d_blocks */
  uint8_t mode;        /* 0 .. getNumModesMip - 1: below 16 (4x4), 8 (a side of 4, or 8x8) or 6 */
  uint8_t transposed;  /* 0 / 1: the input is left | top and the reduced block is transposed (PredictionUnit::mipTransposedFlag) */
  uint8_t reserved[2]; /* 0 */
} vtmhip_mip_job;

/* The trained matrices mipMatrix4x4[16][16][4], mipMatrix8x8[8][16][8] and mipMatrix16x16[6][64][7] (CommonLib/MipData.h; 4 736 bytes) are the caller's data, as
 * LFNST's are: copied to the context's device once; the host arrays may go away afterwards.  The batched entries below return VTMHIP_E_INVALID until it was called. */
int vtmhip_mip_set_tables( vtmhip_ctx *ctx, const uint8_t *m4x4, const uint8_t *m8x8, const uint8_t *m16x16 );

/* predBlock for n (block, mode, transposed) jobs: job k writes width x height samples with stride width at d_predBase + predOff.  Jobs of one block that follow
 * each other in d_jobs share one load of its lines and one pair of reduced boundaries; any order is allowed.
 * NULL pointers, n < 0, numBlocks < 0 and numBlocks == 0 with n > 0 return VTMHIP_E_INVALID; n == 0 is VTMHIP_OK.  The tables stay on the device: a job whose
 * block index is outside [0, numBlocks), whose mode is not below getNumModesMip of its block, whose transposed is above 1, or whose block has a side outside the
 * list, a bitDepth outside 8 .. 12 or multiRefIdx != 0 is skipped -- nothing is read through it and its output is not written.  Lanes per job as for
 * vtmhip_intra_pred_batch_dev (vtmhip_intra_lanes_per_job of the largest well-formed block; no read-back). */
int vtmhip_mip_pred_batch_dev( vtmhip_ctx *ctx, const int16_t *d_refBase, const vtmhip_intra_block *d_blocks, int numBlocks, const vtmhip_mip_job *d_jobs, int n,
                               int16_t *d_predBase );

/* The same prediction formed in LDS and consumed there: d_dist[2 k] = the SAD of job k's prediction against its block's original, d_dist[2 k + 1] = the SATD under
 * the xGetHADs tile rules.  No sample of a prediction goes to global memory; predOff is ignored.  min( 2 * SAD, SATD ), the mode bits and reduceHadCandList stay
 * the caller's.  Checks and skipped jobs as above (both d_dist entries of a skipped job are left). */
int vtmhip_mip_presel_batch_dev( vtmhip_ctx *ctx, const int16_t *d_refBase, const int16_t *d_orgBase, const vtmhip_intra_block *d_blocks, int numBlocks,
                                 const vtmhip_mip_job *d_jobs, int n, uint64_t *d_dist );

/* The same rules on the host, no context: top and left are indexed as the lines of a vtmhip_intra_block are (top[1 .. width] and left[1 .. height] are read, index 0
 * -- the corner -- is not), the matrices as for vtmhip_mip_set_tables, pred receives width x height samples with stride width.  Anything the device would skip, or
 * a NULL pointer, returns VTMHIP_E_INVALID. */
int vtmhip_mip_pred_host( int width, int height, int bitDepth, int mode, int transposed, const int16_t *top, const int16_t *left, const uint8_t *m4x4,
                          const uint8_t *m8x8, const uint8_t *m16x16, int16_t *pred );

int vtmhip_mip_struct_size( int which );   /* sizeof() of 0 vtmhip_mip_job; -1 otherwise */

/* ---- intra luma residual chain: one full-RD level of IntraSearch::estIntraPredLumaQT in one call -- per (mode, transform candidate) the steps of
 * xIntraCodingTUBlock (EncoderLib/IntraSearch.cpp:2989-3320): prediction, piResi.subtract( piPred ), transformNxN / invTransformNxN,
 * piReco.reconstruct( piPred, piResi, clpRng ) and getDistPart( piOrg, piReco, DF_SSE ).  The predictions are the two job tables above with the meaning they have
 * there, over one vtmhip_intra_block table (orgOff / orgStride are used here); the chain is the fused chain of vtmhip_tu_chain_batch_dev.  The only upload of a
 * level is its reference lines and the tables; nothing goes through the host between the steps.
 * The lfnstIdx 1 / 2 candidates of a level go through vtmhip_intra_chain_lfnst_batch_dev below.
 * NOT covered, the caller's or a later change: BDPCM (ISP has an entry of its own, vtmhip_isp_chain_batch_dev below; LFNST with ISP has none); DF_SSE_WTD / LMCS (the caller hands
 * the original in the domain it codes in); RDOQ / dependent quantisation (the chain is Quant::quant, as everywhere in this library); the CABAC bit estimate, the
 * RD decision and the candidate lists; the encoder hook.  The chroma and JCCR intra chains have an entry of their own below (vtmhip_intra_chroma_chain_batch_dev). */
typedef struct
{
  int64_t outOff;            /* W x H contiguous: the levels inside d_levelsBase, the reconstruction inside d_recoBase */
  int32_t pred;              /* 0 .. nIntra - 1: d_intraJobs[pred];  nIntra .. nIntra + nMip - 1: d_mipJobs[pred - nIntra] */
  int16_t qpPer, qpRem;      /* as vtmhip_tu_job */
  uint8_t typeHor, typeVer;  /* VTMHIP_DCT2 / DCT8 / DST7, or both VTMHIP_TRSKIP */
  uint8_t isIRAP, reserved;  /* reserved: 0 */
  int32_t pad;               /* 0 */
} vtmhip_intra_tu_job;

typedef struct
{
  uint64_t sse;              /* DF_SSE of the original block against the clipped reconstruction (xIntraCodingTUBlock :3313) */
  uint64_t sseResi;          /* the chain's own vtmhip_tu_result.sse: residual against reconstructed residual (differs from sse once the clip acts) */
  int32_t  sumAbs, absSum;   /* as vtmhip_tu_result */
} vtmhip_intra_tu_result;

/* Prediction p (p < nIntra: d_intraJobs[p], else d_mipJobs[p - nIntra]) writes its W x H samples with stride W at d_predBase + predOff and the residual
 * original - prediction, same layout, at d_resiBase + predOff -- from the same registers, the original staged on chip; a prediction no TU job names is formed too.
 * TU job k is one transform candidate of prediction `pred`: the block's shape and bit depth, that residual, the job's transform pair and QP.  The chain writes its
 * levels to d_levelsBase + outOff (d_levelsBase may be NULL) and the reconstructed residual to d_recoBase + outOff, which a finish kernel overwrites in place with
 * Clip( prediction + reconstructed residual, 0, ( 1 << bitDepth ) - 1 ); d_results[k].sse is what vtmhip_dist_batch_dev( VTMHIP_DIST_SSE ) gives for the original
 * block and that reconstruction.  Several TU jobs may name one prediction (the MTS candidates of a mode); either prediction table may be empty; nTu == 0 is the
 * prediction + residual pass alone (d_recoBase and d_results may then be NULL).  All counts 0 is VTMHIP_OK.
 * The four tables are read back (one stream synchronisation; never call this under stream capture) and checked on the host before anything is launched; from the
 * same pass come the chain's largest sides, whether every TU job has one size and a real transform (the one-lane and register-blocked chain kernels are then
 * reached without a promise from the caller) and the lanes a prediction gets.  UNLIKE the prediction entries above, which skip a malformed job, this entry
 * REJECTS THE WHOLE CALL -- the chain kernels trust their jobs -- with VTMHIP_E_INVALID and nothing launched: a required pointer NULL, a negative count, MIP jobs
 * before vtmhip_mip_set_tables; any block with a side outside 4 / 8 / 16 / 32 / 64, a bitDepth outside 8 .. 12 or multiRefIdx > 2; a block index outside the
 * table, a mode above 66, planar off line 0; a MIP mode at or above getNumModesMip, transposed > 1, MIP on a block with multiRefIdx != 0; pred outside
 * [0, nIntra + nMip); qpRem outside 0 .. 5, qpPer < 0; a transform pair that is neither two of DCT2 / DCT8 / DST7 nor both VTMHIP_TRSKIP; DST7 / DCT8 on a side
 * above 32, transform skip on a block with a side above 32; a non-zero reserved / pad field in any of the four tables. */
int vtmhip_intra_chain_batch_dev( vtmhip_ctx *ctx, const int16_t *d_refBase, const int16_t *d_orgBase, const vtmhip_intra_block *d_blocks, int numBlocks,
                                  const vtmhip_intra_job *d_intraJobs, int nIntra, const vtmhip_mip_job *d_mipJobs, int nMip, const vtmhip_intra_tu_job *d_tuJobs,
                                  int nTu, int16_t *d_predBase, int16_t *d_resiBase, int32_t *d_levelsBase, int16_t *d_recoBase, vtmhip_intra_tu_result *d_results );

/* The same checks and the same expansion as host arithmetic on host tables, no context: out[k] = TU job k as the fused chain sees it (resiOff = the prediction's
 * predOff inside d_resiBase, resiStride = W).  out holds nTu records and is left untouched when a table is rejected (VTMHIP_E_INVALID).  *maxWidth / *maxHeight: the
 * largest sides over the TU jobs (0 without any); *uniform: 1 when every TU job has one size and a real transform; each of the three may be NULL. */
int vtmhip_intra_chain_make_tu_jobs( const vtmhip_intra_block *blocks, int numBlocks, const vtmhip_intra_job *intraJobs, int nIntra, const vtmhip_mip_job *mipJobs,
                                     int nMip, const vtmhip_intra_tu_job *tuJobs, int nTu, vtmhip_tu_job *out, int *maxWidth, int *maxHeight, int *uniform );

int vtmhip_intra_chain_struct_size( int which );   /* sizeof() of 0 vtmhip_intra_tu_job, 1 vtmhip_intra_tu_result; -1 otherwise */

/* ---- LFNST residual chain: the lfnstIdx 1 / 2 candidates of an intra luma TU in one kernel -- TrQuant::transformNxN / invTransformNxN with cu.lfnstIdx != 0:
 * xT restricted to the kept region (TrQuant.cpp:792-804), xFwdLfnst (:436-526), Quant::quant over the first 8 / 16 scan positions (Quant.cpp:1003-1009),
 * Quant::dequant, xInvLfnst (:339-434), xIT with the same zero-out (:872-884), and the SSE of the residual against the reconstructed residual.  DCT2 in both
 * directions, no transform skip.  The kept primary region is 4x4 when a side is 4 and 8x8 otherwise; 8 scan positions are coded for 4x4 and 8x8 blocks, 16 for
 * every other shape; the bottom-right 4x4 of an 8x8 region carries primary coefficients Quant::quant never reads: zero from there on.  The core matrices are the
 * caller's (vtmhip_lfnst_set_tables).
 * Out of scope: chroma LFNST (separate tree); ISP with LFNST; RDOQ, sign hiding and scaling lists; the CABAC bit estimate; the reference's own LFNST constraints on
 * the coded block (the last-position rule, rapidLFNST); the encoder hook. */
typedef struct
{
  int64_t resiOff, outOff;   /* the residual inside d_resiBase; W x H contiguous: the levels inside d_levelsBase, the reconstructed residual inside d_recBase */
  int32_t resiStride;        /* >= width */
  int16_t width, height;     /* 4, 8, 16, 32, 64 */
  int16_t qpPer, qpRem;      /* as vtmhip_tu_job */
  uint8_t bitDepth, isIRAP;  /* 8 .. 12 */
  uint8_t setIdx, index;     /* lfnstTrSetIdx 0 .. 3 (vtmhip_lfnst_mode_host), lfnstIdx - 1 (0 .. 1) */
  uint8_t transpose;         /* 0 / 1 */
  uint8_t pad[7];            /* 0 */
} vtmhip_lfnst_chain_job;

/* Set index and transpose flag of a prediction on a width x height luma block: PU::getWideAngle, TrQuant::getLFNSTIntraMode / getTransposeFlag and g_lfnstLut for a
 * regular mode 0 .. 66; planar (set 0, no transpose) for a MIP prediction, which needs both sides >= 16 (allowLfnstWithMip); intraMode is ignored then.  Host-only.
 * VTMHIP_E_INVALID: a side outside 4 / 8 / 16 / 32 / 64, a mode outside 0 .. 66, MIP below 16, a NULL pointer. */
int vtmhip_lfnst_mode_host( int width, int height, int intraMode, int isMip, int *setIdx, int *transpose );

/* Per job: d_results[k].sse as vtmhip_tu_chain_batch_dev; sumAbs = sum |coefficient| over the quantised scan positions after the forward LFNST; absSum = uiAbsSum.
 * Levels are W x H contiguous and zero outside the coded positions (d_levelsBase may be NULL); d_recBase may be NULL.  A job gets 16 lanes when the largest job of
 * the table has up to 256 samples and a wave above (vtmhip_lfnst_chain_lanes_per_job).  The table is read back (one stream synchronisation; never under stream
 * capture) and a malformed one REJECTS THE WHOLE CALL with VTMHIP_E_INVALID and nothing launched: a side outside the list, resiStride < width, bitDepth outside
 * 8 .. 12, qpRem outside 0 .. 5, qpPer < 0, setIdx > 3, index > 1, transpose > 1, a non-zero pad byte; also a NULL table, residual or result pointer, n < 0, and
 * a context that has not seen vtmhip_lfnst_set_tables.  n == 0 is VTMHIP_OK. */
int vtmhip_lfnst_chain_batch_dev( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_lfnst_chain_job *d_jobs, int n, int32_t *d_levelsBase, int16_t *d_recBase,
                                  vtmhip_tu_result *d_results );
int vtmhip_lfnst_chain_lanes_per_job( int maxArea );   /* host-only: 16 or 64 */

/* The LFNST candidates of an intra level beside the plain ones: shape and bit depth come from the block, set index and transpose from the prediction. */
typedef struct
{
  int64_t outOff;            /* as vtmhip_intra_tu_job */
  int32_t pred;              /* as vtmhip_intra_tu_job */
  int16_t qpPer, qpRem;      /* as vtmhip_tu_job */
  uint8_t lfnstIdx, isIRAP;  /* 1 .. 2 */
  uint8_t reserved[2];       /* 0 */
  int32_t pad;               /* 0 */
} vtmhip_intra_lfnst_tu_job;   /* its result: vtmhip_intra_tu_result */

/* vtmhip_intra_chain_batch_dev with a second candidate table: the prediction + residual pass runs once, the plain TU jobs go through the fused chain and the LFNST
 * jobs, expanded on the device, through the LFNST chain above; the finish kernel then runs over each result table (clipped reconstruction in place, SSE against the
 * original).  Plain and LFNST jobs may name one prediction; nTu == 0 with nLfnst > 0 is valid, and the reverse; nLfnst == 0 is vtmhip_intra_chain_batch_dev.  All
 * five tables are read back and checked before anything is launched: besides what vtmhip_intra_chain_batch_dev rejects, lfnstIdx outside 1 .. 2, a MIP prediction on
 * a block with a side below 16, pred outside the tables, qpRem outside 0 .. 5, qpPer < 0, a non-zero reserved / pad field, nLfnst < 0, a NULL d_lfnstJobs /
 * d_recoBase / d_lfnstResults with nLfnst > 0, and LFNST jobs before vtmhip_lfnst_set_tables reject the whole call with nothing written. */
int vtmhip_intra_chain_lfnst_batch_dev( vtmhip_ctx *ctx, const int16_t *d_refBase, const int16_t *d_orgBase, const vtmhip_intra_block *d_blocks, int numBlocks,
                                        const vtmhip_intra_job *d_intraJobs, int nIntra, const vtmhip_mip_job *d_mipJobs, int nMip, const vtmhip_intra_tu_job *d_tuJobs,
                                        int nTu, const vtmhip_intra_lfnst_tu_job *d_lfnstJobs, int nLfnst, int16_t *d_predBase, int16_t *d_resiBase,
                                        int32_t *d_levelsBase, int16_t *d_recoBase, vtmhip_intra_tu_result *d_results, vtmhip_intra_tu_result *d_lfnstResults );

/* The same checks and expansion as host arithmetic, no context: outTu[k] as vtmhip_intra_chain_make_tu_jobs, outLfnst[k] = LFNST job k as the LFNST chain sees
 * it.  Both are left untouched when a table is rejected (VTMHIP_E_INVALID).  *maxWidth / *maxHeight / *uniform: over the plain jobs; *lfnstLanes: the lanes an LFNST
 * job gets (0 without any); each of the four may be NULL. */
int vtmhip_intra_chain_lfnst_make_jobs( const vtmhip_intra_block *blocks, int numBlocks, const vtmhip_intra_job *intraJobs, int nIntra, const vtmhip_mip_job *mipJobs,
                                        int nMip, const vtmhip_intra_tu_job *tuJobs, int nTu, const vtmhip_intra_lfnst_tu_job *lfnstJobs, int nLfnst, vtmhip_tu_job *outTu,
                                        vtmhip_lfnst_chain_job *outLfnst, int *maxWidth, int *maxHeight, int *uniform, int *lfnstLanes );

int vtmhip_lfnst_chain_struct_size( int which );   /* sizeof() of 0 vtmhip_lfnst_chain_job, 1 vtmhip_intra_lfnst_tu_job; -1 otherwise */

/* ---- intra chroma residual chain: one full-RD level of IntraSearch::xRecurIntraChromaCodingQT in one call (EncoderLib/IntraSearch.cpp:4934-5260) -- the Cb and Cr
 * predictions of a level and their residuals, then per candidate the chroma branch of xIntraCodingTUBlock (:3196-3318): for a single component scaleSignal( adj, 1 ),
 * transformNxN / invTransformNxN, scaleSignal( adj, 0 ), piReco.reconstruct( piPred, piResi, clpRng ), getDistPart( piOrg, piReco, DF_SSE ); for a joint Cb-Cr
 * candidate scale both, forward ICT, the chain on the coded component, inverse ICT, inverse scaling of both, both reconstructions and both distortions.  The
 * predictions are vtmhip_intra_chroma_job records over a vtmhip_intra_chroma_block table with the meaning they have above (cbOrgOff / crOrgOff / orgStride are used
 * here); the chains are vtmhip_tu_chain_crs_batch_dev and vtmhip_jccr_chain_crs_batch_dev (the plain forms when no job carries an adj).  The reference inverse-scales
 * only when uiAbsSum > 0; a zero block maps to zero, so always doing it is identical.  The only upload of a level is its lines and the tables; nothing goes through
 * the host between the steps.
 * What stays the caller's: the lambda adjustments (:3125-3156); Reshape::calculateChromaAdjVpduNei (the adj comes per job); the cbf-dependent candidate pruning
 * (:5061, :5087, :5179-5224) and selectICTCandidates -- the caller runs the joint candidates speculatively and discards on the host, as for MTS candidates -- ; the
 * discard of a joint candidate whose coded cbf is 0 (:3250-3254: absSum == 0 in the result; the outputs are still written); the CABAC estimate; DF_SSE_WTD under LMCS
 * (the reconstruction is left in global memory, so vtmhip_sse_wtd_batch_dev can follow); BDPCM, LFNST, lossless, ACT; chroma sides of 2; 4:2:2 / 4:4:4. */
typedef struct
{
  int64_t  outOff;          /* W x H contiguous: the levels inside d_levelsBase, the reconstruction inside d_recoBase */
  int32_t  pred;            /* 0 .. nPred - 1: d_jobs[pred] (both components of it were predicted) */
  int16_t  qpPer, qpRem;    /* QpParam( tu, compID ).per / rem; transform skip: per( true ) / rem( true ) */
  uint8_t  component;       /* 0 Cb, 1 Cr */
  uint8_t  typeHor;         /* VTMHIP_DCT2 (DCT2 / DCT2) or VTMHIP_TRSKIP */
  uint8_t  isIRAP, reserved;   /* reserved: 0 */
  uint16_t chromaAdj;       /* tu.getChromaAdj(), 0 = no scaling; at most 32767 */
  uint16_t pad;             /* 0 */
} vtmhip_intra_chroma_tu_job;   /* its result: vtmhip_intra_tu_result */

typedef struct
{
  int64_t  outOff;          /* W x H contiguous: the Cb reconstruction inside d_recoBase, the Cr reconstruction inside d_recoCrBase, the levels of the coded component
                               inside d_levelsBase */
  int32_t  pred;            /* as above */
  int16_t  qpPer, qpRem;    /* QpParam( tu, codeCompId ).per / rem as for vtmhip_jccr_job: the device does not derive it */
  uint8_t  typeHor, isIRAP; /* typeHor: VTMHIP_DCT2 or VTMHIP_TRSKIP */
  uint8_t  cbfMask;         /* tu.jointCbCr: 1 .. 3 */
  uint8_t  signFlag;        /* picHeader.getJointCbCrSignFlag(): 0 / 1 */
  uint16_t chromaAdj, pad;  /* as above */
} vtmhip_intra_chroma_joint_job;

typedef struct
{
  uint64_t sseCb, sseCr;          /* DF_SSE of the original blocks against the clipped reconstructions (:3313-3316) */
  uint64_t sseResiCb, sseResiCr;  /* the joint chain's own vtmhip_jccr_result.sseCb / sseCr: residual against reconstructed residual */
  int64_t  fwdDist;               /* as vtmhip_jccr_result */
  int32_t  sumAbs, absSum;        /* as vtmhip_jccr_result; absSum == 0: the reference discards this candidate (:3250) */
} vtmhip_intra_chroma_joint_result;

/* Prediction p (d_jobs[p]) writes its Cb and Cr samples with stride W at d_predBase + cbPredOff / crPredOff and the UNSCALED residuals original - prediction, same
 * layout, at the same offsets inside d_resiBase (the chains scale on load) -- from the same registers, the two originals staged on chip; a prediction no job names
 * is formed too.  Single job k is one transform candidate of one component of prediction `pred`; joint job k one (cbfMask, transform) candidate of it.  Several jobs
 * may name one prediction (Cb DCT2, Cb TS, Cr DCT2, Cr TS, three masks times two transforms).  The chains write the levels to d_levelsBase + outOff (d_levelsBase may
 * be NULL) and the reconstructed residuals to d_recoBase / d_recoCrBase + outOff, which a finish kernel overwrites in place with
 * Clip( prediction + reconstructed residual, 0, ( 1 << bitDepth ) - 1 ); sse / sseCb / sseCr are what vtmhip_dist_batch_dev( VTMHIP_DIST_SSE ) gives for the original
 * block and that reconstruction.  nTu == nJoint == 0 is the prediction + residual pass alone; a table that is empty needs none of its pointers (d_recoBase serves
 * both job tables, d_recoCrBase the joint one); d_lumaBase may be NULL when no job of d_jobs is an LM mode.  All of nPred, nTu, nJoint 0 is VTMHIP_OK.
 * The four tables are read back (one stream synchronisation; never call this under stream capture) and checked on the host before anything is launched; from the
 * same pass come the lanes a prediction gets, per job table the largest sides and whether all its jobs have one size and VTMHIP_DCT2 (the one-lane and
 * register-blocked chain kernels are then reached without a promise from the caller), and whether any job carries an adj.  As vtmhip_intra_chain_batch_dev, and
 * UNLIKE the prediction entries above, this entry REJECTS THE WHOLE CALL with VTMHIP_E_INVALID and nothing launched: a required pointer NULL, a negative count; a
 * block the prediction entries would skip (a side outside 4 / 8 / 16 / 32, a bitDepth outside 8 .. 12, a flag above 1, inconsistent availability); a block index
 * outside the table, a mode above 69, an LM mode without d_lumaBase; pred outside [0, nPred); component > 1; typeHor other than VTMHIP_DCT2 / VTMHIP_TRSKIP; qpRem
 * outside 0 .. 5, qpPer < 0; chromaAdj > 32767; cbfMask outside 1 .. 3; signFlag > 1; a non-zero reserved / pad field in any of the four tables. */
int vtmhip_intra_chroma_chain_batch_dev( vtmhip_ctx *ctx, const int16_t *d_refBase, const int16_t *d_lumaBase, const int16_t *d_orgBase,
                                         const vtmhip_intra_chroma_block *d_blocks, int numBlocks, const vtmhip_intra_chroma_job *d_jobs, int nPred,
                                         const vtmhip_intra_chroma_tu_job *d_tuJobs, int nTu, const vtmhip_intra_chroma_joint_job *d_jointJobs, int nJoint,
                                         int16_t *d_predBase, int16_t *d_resiBase, int32_t *d_levelsBase, int16_t *d_recoBase, int16_t *d_recoCrBase,
                                         vtmhip_intra_tu_result *d_results, vtmhip_intra_chroma_joint_result *d_jointResults );

/* The same checks and the same expansion as host arithmetic on host tables, no context: outTu[k] = single job k as vtmhip_tu_chain_crs_batch_dev sees it (resiOff =
 * the component's prediction offset inside d_resiBase, resiStride = W), outJoint[k] = joint job k as vtmhip_jccr_chain_crs_batch_dev sees it (cbOff / crOff = the two
 * prediction offsets).  outTu holds nTu and outJoint nJoint records; both are left untouched when a table is rejected (VTMHIP_E_INVALID).  maxWidth / maxHeight:
 * int[2] each -- [0] over the single jobs, [1] over the joint jobs: the largest sides (0 without any job); *uniformTu / *uniformJoint: 1 when every job of that
 * table has one size and VTMHIP_DCT2; *crs: 1 when some job of either table has a non-zero chromaAdj.  Each of the five may be NULL. */
int vtmhip_intra_chroma_chain_make_jobs( const vtmhip_intra_chroma_block *blocks, int numBlocks, const vtmhip_intra_chroma_job *jobs, int nPred,
                                         const vtmhip_intra_chroma_tu_job *tuJobs, int nTu, const vtmhip_intra_chroma_joint_job *jointJobs, int nJoint,
                                         vtmhip_tu_job *outTu, vtmhip_jccr_job *outJoint, int *maxWidth, int *maxHeight, int *uniformTu, int *uniformJoint, int *crs );

int vtmhip_intra_chroma_chain_struct_size( int which );   /* sizeof() of 0 vtmhip_intra_chroma_tu_job, 1 vtmhip_intra_chroma_joint_job, 2 vtmhip_intra_chroma_joint_result; -1 otherwise */

/* ---- intra sub-partitions (ISP), luma: one (CU, intra mode, split direction) candidate per job, every sub-partition of it in one kernel -- per sub-partition the
 * steps of IntraSearch::xIntraCodingTUBlock with cu.ispMode set (EncoderLib/IntraSearch.cpp:2989-3320): the prediction of its region from the reconstruction of the
 * one before (initIntraPatternChTypeISP, CommonLib/IntraPrediction.cpp:802-918), residual, xT -> Quant::quant -> Quant::dequant -> xIT with the ISP transform pair
 * (DST7 on a side of 4 .. 16, else DCT2; TrQuant.cpp:713-724) on TUs down to 1 x N and N x 1, the clipped reconstruction and its SSE.  Nothing of a candidate touches
 * global memory between the load of its lines and original and the final stores.  The rules have one definition for host and device, vtm_amd/csrc/isp_rules.hpp.
 * Scope: lfnstIdx 0, multiRefIdx 0, the regular modes 0 .. 66 (the reference forbids MIP and MRL with ISP, IntraSearch.cpp:1049-1050), every CU shape CU::canUseISP
 * admits with MaxTbSize 64 (sides 4 .. 64 without 4x4), 8 .. 12 bits, Quant::quant with the flat list.
 * Stays the caller's: the early exits of xIntraCodingLumaISP (IntraSearch.cpp:3516-3553; they need bits, so the device always codes every sub-partition); the bit
 * estimate; the "at least one non-zero CBF" rule (:3173; absSum is reported per sub-partition); the candidate list (xSortISPCandList / xGetNextISPMode); LFNST with
 * ISP; the availability analysis that fills the CU's first lines. */
typedef struct
{
  int32_t numParts, partW, partH;    /* the sub-partitions (TUs): 2 for 4x8 / 8x4, else 4 */
  int32_t numRegions, regW, regH;    /* the prediction regions: the TUs, except 4 wide under a vertical split of a CU of width 4, or of width 8 and height > 4 */
  int32_t typeHor, typeVer;          /* the transform pair of a TU (VTMHIP_DCT2 / VTMHIP_DST7; a side of 1 is not transformed) */
} vtmhip_isp_geom;

typedef struct
{
  int64_t predOff;      /* the assembled W x H prediction (stride W) inside d_predBase */
  int64_t outOff;       /* the W x H reconstruction (stride W) inside d_recoBase; the levels of sub-partition k, one contiguous partW x partH block, at
                           outOff + k * partW * partH inside d_levelsBase */
  int32_t block;        /* index into d_blocks (a vtmhip_intra_block with multiRefIdx 0; its lines: 2W + 1 and 2H + 1 samples) */
  int16_t qpPer, qpRem; /* as vtmhip_tu_job */
  uint8_t mode;         /* 0 planar, 1 DC, 2 .. 66 */
  uint8_t split;        /* 1 horizontal (rows), 2 vertical (columns): ISPType */
  uint8_t sideAvail;    /* the left (horizontal split) or above (vertical split) neighbour of the CU exists: the branch of the line update (IntraPrediction.cpp:849, 880) */
  uint8_t isIRAP;
  uint8_t reserved[4];  /* 0 */
} vtmhip_isp_job;

typedef struct
{
  uint64_t sse[4];      /* per sub-partition: DF_SSE of the original against the clipped reconstruction */
  int32_t  absSum[4];   /* as vtmhip_tu_result, per sub-partition (cbf = absSum > 0) */
  int32_t  sumAbs[4];
  int32_t  numParts;    /* entries past numParts are 0 */
  int32_t  reserved;    /* 0 */
} vtmhip_isp_result;

/* n ISP candidates over the block table of vtmhip_intra_pred_batch_dev (orgOff / orgStride are used).  Job k writes its W x H reconstruction at d_recoBase + outOff,
 * its levels at d_levelsBase + outOff (d_levelsBase may be NULL), its assembled prediction at d_predBase + predOff (d_predBase may be NULL) and d_results[k].  A job
 * gets 16 / 64 / 256 lanes by the largest CU the jobs name (vtmhip_intra_lanes_per_job), 256 also where four jobs would not fit the workgroup's LDS (a 64-point
 * transform among the jobs).  Both tables are read back and checked before anything runs (one stream synchronisation; never under stream capture): a shape
 * canUseISP refuses, a bitDepth outside 8 .. 12, multiRefIdx != 0, a mode above 66, split outside 1 .. 2, sideAvail / isIRAP above 1, qpRem outside 0 .. 5,
 * qpPer < 0, a non-zero reserved field or a block index outside the table reject the whole call with VTMHIP_E_INVALID and nothing written; so do NULL d_refBase /
 * d_orgBase / d_blocks / d_jobs / d_recoBase / d_results with n > 0, n < 0 and numBlocks < 0.  n == 0 is VTMHIP_OK. */
int vtmhip_isp_chain_batch_dev( vtmhip_ctx *ctx, const int16_t *d_refBase, const int16_t *d_orgBase, const vtmhip_intra_block *d_blocks, int numBlocks,
                                const vtmhip_isp_job *d_jobs, int n, int16_t *d_predBase, int32_t *d_levelsBase, int16_t *d_recoBase, vtmhip_isp_result *d_results );

/* The same rules on the host, no context (VTMHIP_E_INVALID for anything outside the scope above).
 * vtmhip_isp_geometry: CU::getISPSplitDim and the prediction regions of a width x height CU under `split`.
 * vtmhip_isp_pred_params: m_ipaParam of a regW x regH prediction region of a cuW x cuH CU -- the wide-angle shift from the CU, PDPC and angularScale from the region,
 * no filter of either kind.
 * vtmhip_isp_tr_types: the transform pair of a partW x partH TU.
 * vtmhip_isp_pred_region_host: predIntraAng of one region from given lines, top[0 .. cuW + regW] and left[0 .. cuH + regH]; pred: regW x regH, stride regW.
 * vtmhip_isp_next_lines_host: the lines region `region` >= 1 sees, from the CU's lines (2W + 1 and 2H + 1 samples) and a reconstruction (W x H, stride W) of which
 * the row above / the column left of the region is read: topOut[0 .. cuW + regW], leftOut[0 .. cuH + regH].
 * vtmhip_isp_chain_host: vtmhip_isp_chain_batch_dev as host arithmetic over host tables, same checks, same outputs (predBase and levelsBase may be NULL). */
int vtmhip_isp_geometry( int width, int height, int split, vtmhip_isp_geom *out );
int vtmhip_isp_pred_params( int cuW, int cuH, int regW, int regH, int mode, vtmhip_intra_params *out );
int vtmhip_isp_tr_types( int partW, int partH, int *typeHor, int *typeVer );
int vtmhip_isp_pred_region_host( int cuW, int cuH, int regW, int regH, int mode, int bitDepth, const int16_t *top, const int16_t *left, int16_t *pred );
int vtmhip_isp_next_lines_host( int cuW, int cuH, int split, int region, int sideAvail, const int16_t *top, const int16_t *left, const int16_t *reco, int16_t *topOut,
                                int16_t *leftOut );
int vtmhip_isp_chain_host( const int16_t *refBase, const int16_t *orgBase, const vtmhip_intra_block *blocks, int numBlocks, const vtmhip_isp_job *jobs, int n,
                           int16_t *predBase, int32_t *levelsBase, int16_t *recoBase, vtmhip_isp_result *results );
/* the lanes a job of these (host) tables gets, after the same checks: 16, 64 or 256 */
int vtmhip_isp_chain_lanes_host( const vtmhip_intra_block *blocks, int numBlocks, const vtmhip_isp_job *jobs, int n, int *lanes );
int vtmhip_isp_struct_size( int which );   /* sizeof() of 0 vtmhip_isp_job, 1 vtmhip_isp_result, 2 vtmhip_isp_geom; -1 otherwise */

#ifdef __cplusplus
}
#endif
#endif /* VTMHIP_H */
