// mest_glue.hpp -- the per-row bookkeeping of InterSearch::xMotionEstimation (reference EncoderLib/InterSearch.cpp:3299-3494) as device functions, shared by
//   * the stand-alone glue kernels of mest.hip (mixed batches: one thread per row turns one stage's results into the next stage's job records), and
//   * the FUSED forms of the search kernels (round 4): tz_search_kernel / full_search_sq_kernel / frac_search_*_kernel derive their job records from the
//     xMotionEstimation rows themselves in a prologue (a record in LDS, built by one lane of the job's workgroup) and frac_search_* writes the row's final result in its
//     epilogue -- the one-thread-per-row launches between the searches (amvp_select, mest_prepare, mest_mid, mest_final: 232-byte records moved at HBM speed, and a launch each on
//     the dependent chain of a level / of a CU-level call) disappear for uniform batches.
// One source for both, so that the fused and the stand-alone forms cannot drift apart; the motion-vector rules themselves are in mv_rules.hpp.
#pragma once
#include "ctx.hpp"
#include "mv_rules.hpp"

namespace mg
{

__device__ __forceinline__ void clip_mv( const vtmhip_pic_params &pic, const vtmhip_me_job &j, int &hor, int &ver )   // clipMvInPic (Mv.cpp:56-74)
{
  const int horMax = MVR_CLIP_MAX( pic.picW, j.puX ), horMin = MVR_CLIP_MIN( pic.ctuSize, j.puX );
  const int verMax = MVR_CLIP_MAX( pic.picH, j.puY ), verMin = MVR_CLIP_MIN( pic.ctuSize, j.puY );
  hor = min( horMax, max( horMin, hor ) );
  ver = min( verMax, max( verMin, ver ) );
}
__device__ __forceinline__ int sub_shift( const vtmhip_me_cfg &cfg, int w, int h ) { return cfg.fastInterSearchMode13 && h > 8 && w <= 64 ? 1 : 0; }   // RdCost.cpp:289-323, mode 2
__host__ inline int            sub_shift( const vtmhip_me_cfg &cfg, int w, int h ) { return cfg.fastInterSearchMode13 && h > 8 && w <= 64 ? 1 : 0; }   // the host's copy (launch code)
// CU-level BCW weight of the searched list of a bi job (0: the default pair); the default weight (4 of 8) is normalised to 0
__device__ __forceinline__ int bcw_weight( const vtmhip_me_job &j ) { const int w = j.bi ? VTMHIP_MEJ_BCW_WEIGHT( j.flags ) : 0; return w == 4 ? 0 : w; }

// m_uniMvList entry i (newest first) is kept only if no earlier entry equals it (:3391-3403, :3728-3746).  No local array: a run-time indexed one would live in scratch
// memory, and a kernel with scratch pays for its set-up at every launch (mest_prepare_kernel: 18 us per launch for a handful of rows in the round-3 traces)
__device__ __forceinline__ bool extra_is_first( const vtmhip_me_job &j, int i )
{
  for( int k = 0; k < i; k++ ) if( j.extraStart[k][0] == j.extraStart[i][0] && j.extraStart[k][1] == j.extraStart[i][1] ) return false;
  return true;
}
__device__ __forceinline__ int num_extra( const vtmhip_me_job &j ) { return min( 15, max( 0, j.numExtraStart ) ); }

// the xTZSearch job of a uni row (:3434-3447); `slot` / `slotStride`: where the search pattern (the original block) sits.  _scalars: everything but the start-candidate list
// (predH / predV: the row's predictor -- j.mvPredHor / mvPredVer, or the AMVP selection a fused prologue has just made)
__device__ __forceinline__ void make_tz_job_scalars( const vtmhip_me_cfg &cfg, const vtmhip_me_job &j, long slot, int slotStride, int predH, int predV, vtmhip_tz_job &t )
{
  t.orgOff = slot; t.refOff = j.refOff; t.orgStride = slotStride; t.refStride = j.refStride;
  t.puX = j.puX; t.puY = j.puY; t.width = j.width; t.height = j.height; t.subShift = ( int16_t ) sub_shift( cfg, j.width, j.height ); t.imvShift = ( uint8_t ) mvr::imv_shift( j.imv );
  t.signedSamples = 0;
  t.predHor = mvr::prec_down( predH, 2 ); t.predVer = mvr::prec_down( predV, 2 ); t.motionLambda = j.motionLambda;
  const bool cached = ( j.flags & VTMHIP_MEJ_CACHED_INT_MV ) != 0;   // block-vector cache hit (:3360-3368): rcMv = the cached vector, xTZSearch with bFastSettings (:3434-3441)
  t.mvHor = cached ? j.mvHor : predH; t.mvVer = cached ? j.mvVer : predV;   // else rcMv = rcMvPred (:3446)
  t.searchRange = j.searchRange;
  t.extendedSettings = cfg.extendedSettings; t.fastSettings = cached; t.firstSearchStop = cfg.firstSearchStop; t.hasIntMv2Nx2NPred = 0;
  t.intMv2Nx2NPredHor = t.intMv2Nx2NPredVer = 0;
}
__device__ __forceinline__ void make_tz_job( const vtmhip_me_cfg &cfg, const vtmhip_me_job &j, long slot, int slotStride, vtmhip_tz_job &t )
{
  make_tz_job_scalars( cfg, j, slot, slotStride, j.mvPredHor, j.mvPredVer, t );
  int nex = 0;
  const int m = num_extra( j );
  for( int i = 0; i < m; i++ )
    if( extra_is_first( j, i ) ) { t.extraStart[nex][0] = j.extraStart[i][0]; t.extraStart[nex][1] = j.extraStart[i][1]; nex++; }
  t.numExtraStart = nex;
}

// the exhaustive-search job of a bi row around `centerHor / centerVer` (xSetSearchRange + xPatternSearch, :3421-3432)
__device__ __forceinline__ void make_full_job( const vtmhip_me_cfg &cfg, const vtmhip_me_job &j, long slot, int slotStride, int centerHor, int centerVer, vtmhip_full_job &f )
{
  f.orgOff = slot; f.refOff = j.refOff; f.orgStride = slotStride; f.refStride = j.refStride;
  f.puX = j.puX; f.puY = j.puY; f.width = j.width; f.height = j.height; f.subShift = ( int16_t ) sub_shift( cfg, j.width, j.height );
  f.imvShift = ( uint8_t ) mvr::imv_shift( j.imv ); f.signedSamples = 1;
  f.predHor = mvr::prec_down( j.mvPredHor, 2 ); f.predVer = mvr::prec_down( j.mvPredVer, 2 ); f.motionLambda = j.motionLambda; f.centerHor = centerHor; f.centerVer = centerVer;
  f.searchRange = cfg.bipredSearchRange; f.pad = 0;
}

// the xPatternSearchFracDIF job of a row with cu.imv 0 / IMV_HPEL (:3459-3475)
__device__ __forceinline__ void make_frac_job( int useHadME, int bitDepth, const vtmhip_me_job &j, int intX, int intY, long slot, int slotStride, vtmhip_frac_job &q )
{
  q.orgOff = slot; q.refOff = j.refOff; q.orgStride = slotStride; q.refStride = j.refStride; q.width = j.width; q.height = j.height;
  q.intX = ( int16_t ) intX; q.intY = ( int16_t ) intY;
  q.predHor = mvr::prec_down( j.mvPredHor, 2 ); q.predVer = mvr::prec_down( j.mvPredVer, 2 ); q.motionLambda = j.motionLambda;
  q.useHad = ( uint8_t ) useHadME; q.useAltHpelIf = j.imv == 3; q.imvShift = j.imv == 3; q.bitDepth = ( uint8_t ) bitDepth; q.wideOrg = bcw_weight( j ) != 0;
}

// the rate re-weighting after the fractional search (:3476-3485): the row's result
__device__ __forceinline__ void make_out_frac( const vtmhip_me_job &j, int intX, int intY, unsigned long long intDist, const vtmhip_frac_result &f, vtmhip_me_out &o )
{
  const double fWeight = mvr::me_dist_weight( j.bi, bcw_weight( j ), 0 );
  const double lam = j.motionLambda;
  o.intX = intX; o.intY = intY; o.intDist = intDist;
  const int      qx = ( intX << 2 ) + ( f.halfX << 1 ) + f.qterX, qy = ( intY << 2 ) + ( f.halfY << 1 ) + f.qterY;
  const unsigned mvBits = mvr::mv_bits( qx, qy, mvr::prec_down( j.mvPredHor, 2 ), mvr::prec_down( j.mvPredVer, 2 ), 0, mvr::imv_shift( j.imv ) );
  const unsigned bits = j.bits + mvBits;
  o.cost = ( unsigned long long ) ( floor( fWeight * ( ( double ) f.cost - ( double ) mvr::rate( lam, mvBits ) ) ) + ( double ) mvr::rate( lam, bits ) );   // :3483
  o.mvHor = qx << 2; o.mvVer = qy << 2; o.mvPredHor = j.mvPredHor; o.mvPredVer = j.mvPredVer; o.mvpIdx = j.mvpIdx; o.bits = bits;
}

}   // namespace mg

// What a fused search kernel gets beside (instead of) its own job table.  me == nullptr: not fused (the kernel reads its job table as before).
struct MeFuse
{
  vtmhip_me_job            *me;          // the xMotionEstimation rows of the batch (written only by the AMVP selection)
  const unsigned long long *amvpDout;    // tz: [2 * row + c] template SADs of the AMVP candidates -> xEstimateMvPredAMVP's selection in the prologue (nullptr: rows already chosen)
  unsigned long long       *distBiP;     //     [row] *puiDistBiP (may be nullptr)
  int                       addIdxBits;  //     the chosen predictor's index bits join the row's bits (predInterSearch :2381)
  const vtmhip_me_result   *ires;        // frac: the integer stage's results
  vtmhip_me_out            *out;         // frac: the row's final record, written in the epilogue
  vtmhip_tz_job            *tzSpill;     // tz, split launches: the LDS-built job of a search that goes to the raster kernel is stored here (that kernel and the resume launch read it)
  const int16_t            *biBase;      // (unused by kernels: host bookkeeping)
  vtmhip_me_cfg             cfg;
  int                       bitDepth;
  int                       patIsOther;  // 0: the search pattern is the row's original block (orgOff / orgStride); 1: the caller-made bi-pred target (otherPredOff / otherPredStride)
};
__device__ __forceinline__ long fuse_pat_off( const MeFuse &F, const vtmhip_me_job &j ) { return F.patIsOther ? j.otherPredOff : j.orgOff; }
__device__ __forceinline__ int  fuse_pat_stride( const MeFuse &F, const vtmhip_me_job &j ) { return F.patIsOther ? j.otherPredStride : j.orgStride; }

// the slim view a fused fractional-search kernel takes (kernel arguments live in scalar registers for the kernel's whole life: only what it needs)
struct FracFuse
{
  const vtmhip_me_job    *me;      // nullptr: not fused
  const vtmhip_me_result *ires;
  vtmhip_me_out          *out;
  int                     useHadME, bitDepth, patIsOther;
};
__device__ __forceinline__ long fuse_pat_off( const FracFuse &F, const vtmhip_me_job &j ) { return F.patIsOther ? j.otherPredOff : j.orgOff; }
__device__ __forceinline__ int  fuse_pat_stride( const FracFuse &F, const vtmhip_me_job &j ) { return F.patIsOther ? j.otherPredStride : j.orgStride; }

// the view a fused exhaustive-search kernel takes: the bi rows; noStart: rcMv is the search centre (empty m_uniMvList lists), else the kernel evaluates the start candidates
// (rcMv + the distinct m_uniMvList entries, :3377-3420) itself
struct FullFuse
{
  const vtmhip_me_job *me;      // nullptr: not fused
  int                  subShiftMode13, bipredSearchRange, patIsOther, noStart;
};
__device__ __forceinline__ long fuse_pat_off( const FullFuse &F, const vtmhip_me_job &j ) { return F.patIsOther ? j.otherPredOff : j.orgOff; }
__device__ __forceinline__ int  fuse_pat_stride( const FullFuse &F, const vtmhip_me_job &j ) { return F.patIsOther ? j.otherPredStride : j.orgStride; }
namespace mg
{
__device__ __forceinline__ void make_full_job( const FullFuse &F, const vtmhip_me_job &j, int centerHor, int centerVer, vtmhip_full_job &f )
{
  vtmhip_me_cfg c; c.fastInterSearchMode13 = ( uint8_t ) F.subShiftMode13; c.bipredSearchRange = F.bipredSearchRange;
  make_full_job( c, j, fuse_pat_off( F, j ), fuse_pat_stride( F, j ), centerHor, centerVer, f );
}
}

