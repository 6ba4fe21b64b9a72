// mmvd_rules.hpp -- the rules of the MMVD merge candidates of the reference, defined once for host and device: plain integer functions without a HIP dependency, so
// host/test_mmvd.cpp compiles them with g++ and the kernels of mmvd.hip use the same text.
//   mmvdOffset / mmvdTested      the step table and the candidate loop                              CommonLib/ContextModelling.cpp:359-378, EncoderLib/EncCu.cpp:2528-2534
//   mmvdDistScaleFactor          PU::getDistScaleFactor (xGetDistScaleFactor)                       CommonLib/UnitTools.cpp:1361-1378, :1415
//   mmvdScaleMv                  Mv::scaleMv, one component                                         CommonLib/Mv.h:176-181
//   mmvdStorageClip              Mv::clipToStorageBitDepth, one component                           CommonLib/Mv.h:259-263
//   mmvdSecondOffset             the offset of the list that does not carry the step of a bi base   CommonLib/ContextModelling.cpp:403-445
//   mmvdEqDistOppositePoc        PU::isBiPredFromDifferentDirEqDistPoc                              CommonLib/UnitTools.cpp:3239-3260
//   mmvdClipMin / Max / Axis     clipMvInPic                                                        CommonLib/Mv.cpp:56-74 (mv_rules.hpp has the device's; mmvd.hip asserts they agree)
//   mmvdDerive                   MergeCtx::setMmvdMergeCandiInfo + PU::restrictBiPredMergeCandsOne, the kind of prediction InterPrediction::xPredInterBi picks
//                                under the loop's mmvdEncOptMode and the vectors it predicts with    :355-528, UnitTools.cpp:3262-3274, InterPrediction.cpp:527-572, :240-272
//   mmvdJobOk                    what a row of vtmhip_mmvd_cand_satd_batch_dev's table must satisfy, shared with vtmhip_mmvd_cands_host
#pragma once
#include <stdint.h>

#include "../../include/vtmhip.h"

#if defined( __HIPCC__ )
#define MMVD_HD __host__ __device__ inline
#else
#define MMVD_HD inline
#endif

enum { MMVD_REFINE_STEP = 8, MMVD_MAX_REFINE_NUM = 32, MMVD_BDOF_STEPS = 3, MMVD_BDOF_MAX = 24, MMVD_BCW_DEFAULT = 4 };
enum { MMVD_PRED_L0 = 0, MMVD_PRED_L1 = 1, MMVD_PRED_BI = 2 };   // vtmhip_pred_job::mode

MMVD_HD int mmvdClip3( int lo, int hi, int v ) { return v < lo ? lo : v > hi ? hi : v; }
MMVD_HD int mmvdAbs( int v ) { return v < 0 ? -v : v; }

MMVD_HD int mmvdBase( int cand ) { return cand / MMVD_MAX_REFINE_NUM; }
MMVD_HD int mmvdStep( int cand ) { return ( cand % MMVD_MAX_REFINE_NUM ) / 4; }
MMVD_HD int mmvdPos( int cand ) { return cand & 3; }

// refMvdCands[step], << 2 under picHeader.getDisFracMMVD(): 1/16 units
MMVD_HD int mmvdOffset( int step, int disFrac ) { return ( ( 1 << step ) << 2 ) << ( disFrac ? 2 : 0 ); }

// the loop of EncCu::xCheckRDCostMerge2Nx2N: tempNum candidates, those of a step >= MmvdDisNum skipped
MMVD_HD bool mmvdTested( int numBase, int numSteps, int cand ) { return cand >= 0 && cand < numBase * MMVD_MAX_REFINE_NUM && mmvdStep( cand ) < numSteps; }

// xGetDistScaleFactor( currPOC, currRefPOC, colPOC, colRefPOC ) with diffB = currPOC - currRefPOC, diffD = colPOC - colRefPOC (diffD != 0 unless equal to diffB)
MMVD_HD int mmvdDistScaleFactor( int diffB, int diffD )
{
  if( diffD == diffB ) return 4096;
  const int tdb = mmvdClip3( -128, 127, diffB ), tdd = mmvdClip3( -128, 127, diffD );
  const int x   = ( 0x4000 + mmvdAbs( tdd / 2 ) ) / tdd;
  return mmvdClip3( -4096, 4095, ( tdb * x + 32 ) >> 6 );
}

MMVD_HD int mmvdStorageClip( int v ) { return mmvdClip3( -( 1 << 17 ), ( 1 << 17 ) - 1, v ); }
MMVD_HD int mmvdScaleMv( int scale, int v ) { return mmvdStorageClip( ( scale * v + 128 - ( scale * v >= 0 ) ) >> 8 ); }   // MV_MIN / MV_MAX are the storage limits

// A bi base with unequal POC differences: the list whose picture is further from the current one carries the offset -- list 1 iff |d1| > |d0|, so list 0 on equal
// distances of opposite sides.  mmvdSecondOffset: the other list's offset component for the carrier's component v (the same v on equal differences).
MMVD_HD int mmvdCarrier( int pocDiff0, int pocDiff1 ) { return mmvdAbs( pocDiff1 ) > mmvdAbs( pocDiff0 ) ? 1 : 0; }
MMVD_HD int mmvdSecondOffset( int pocDiff0, int pocDiff1, int anyLongTerm, int v )
{
  if( pocDiff0 == pocDiff1 ) return v;
  if( anyLongTerm ) return ( long long ) pocDiff1 * pocDiff0 > 0 ? v : -v;
  const int carrier = mmvdCarrier( pocDiff0, pocDiff1 );
  // getDistScaleFactor( cur, pocOther, cur, pocCarrier ): diffB = cur - pocOther, diffD = cur - pocCarrier
  return mmvdScaleMv( mmvdDistScaleFactor( carrier ? -pocDiff0 : -pocDiff1, carrier ? -pocDiff1 : -pocDiff0 ), v );
}

MMVD_HD bool mmvdEqDistOppositePoc( int pocDiff0, int pocDiff1, int anyLongTerm )
{
  return !anyLongTerm && ( long long ) pocDiff0 * pocDiff1 < 0 && mmvdAbs( pocDiff0 ) == mmvdAbs( pocDiff1 );
}

// clipMvInPic: the limits of a vector component (1/16) of a CU at luma position pos; size: the picture's width (height)
constexpr int mmvdClipMax( int size, int pos ) { return ( size + 8 - pos - 1 ) << 4; }
constexpr int mmvdClipMin( int ctuSize, int pos ) { return ( -ctuSize - 8 - pos + 1 ) * 16; }
MMVD_HD int mmvdClipAxis( int v, int size, int ctuSize, int pos ) { return mmvdClip3( mmvdClipMin( ctuSize, pos ), mmvdClipMax( size, pos ), v ); }

MMVD_HD bool mmvdBcwOk( int w ) { return w == -2 || w == 3 || w == 4 || w == 5 || w == 10; }
MMVD_HD bool mmvdSideOk( int s ) { return s >= 4 && s <= 128 && ( s & ( s - 1 ) ) == 0; }

MMVD_HD bool mmvdBaseOk( const vtmhip_mmvd_base &b, int width )
{
  if( b.refIdx[0] < 0 && b.refIdx[1] < 0 ) return false;
  for( int l = 0; l < 2; l++ )
    if( b.refIdx[l] >= 0 && b.refStride[l] < width ) return false;
  return mmvdBcwOk( b.bcwWeightL1 );
}

MMVD_HD bool mmvdJobOk( const vtmhip_mmvd_job &j )
{
  if( !mmvdSideOk( j.width ) || !mmvdSideOk( j.height ) || ( j.width == 4 && j.height == 4 ) ) return false;
  if( j.numBase < 1 || j.numBase > 2 || j.numSteps < 1 || j.numSteps > MMVD_REFINE_STEP ) return false;
  if( j.bitDepth < 8 || j.bitDepth > 12 || j.orgStride < j.width ) return false;
  for( int b = 0; b < j.numBase; b++ )
    if( !mmvdBaseOk( j.base[b], j.width ) ) return false;
  return true;
}

// the BDOF condition of a base's candidates up to step MMVD_BDOF_STEPS - 1 (it does not depend on pos): what decides the number of expansion rows
MMVD_HD bool mmvdBaseBdof( const vtmhip_mmvd_job &j, int b )
{
  const vtmhip_mmvd_base &s = j.base[b];
  return j.bdofAllowed && s.refIdx[0] >= 0 && s.refIdx[1] >= 0 && j.width + j.height != 12 && mmvdEqDistOppositePoc( s.pocDiff[0], s.pocDiff[1], s.longTerm[0] | s.longTerm[1] ) &&
         j.width >= 8 && j.height >= 8 && j.width * j.height >= 128 && s.bcwWeightL1 == MMVD_BCW_DEFAULT;
}
MMVD_HD int mmvdNumBdof( const vtmhip_mmvd_job &j )
{
  int n = 0;
  for( int b = 0; b < j.numBase; b++ )
    if( mmvdBaseBdof( j, b ) ) n += 4 * ( j.numSteps < MMVD_BDOF_STEPS ? j.numSteps : MMVD_BDOF_STEPS );
  return n;
}
MMVD_HD int mmvdNumTested( const vtmhip_mmvd_job &j ) { return j.numBase * j.numSteps * 4; }

// One candidate of a job that mmvdJobOk accepts.  out: the record; predMode: MMVD_PRED_*; predMv: the clipped vectors of the lists the prediction reads (0 elsewhere).
MMVD_HD void mmvdDerive( const vtmhip_mmvd_job &j, int picW, int picH, int ctuSize, int cand, vtmhip_mmvd_cand &out, int &predMode, int32_t predMv[2][2] )
{
  out.mv[0][0] = out.mv[0][1] = out.mv[1][0] = out.mv[1][1] = 0;
  out.refIdx[0] = out.refIdx[1] = -1;
  out.interDir = 0; out.bcwWeightL1 = 0; out.useAltHpelIf = 0; out.kind = VTMHIP_MMVD_NOT_TESTED; out.pad[0] = out.pad[1] = 0;
  predMode = MMVD_PRED_L0;
  predMv[0][0] = predMv[0][1] = predMv[1][0] = predMv[1][1] = 0;
  if( !mmvdTested( j.numBase, j.numSteps, cand ) ) return;

  const int               b = mmvdBase( cand ), step = mmvdStep( cand ), pos = mmvdPos( cand );
  const vtmhip_mmvd_base &s = j.base[b];
  const int  offset = mmvdOffset( step, j.disFracMmvd ), sgn = ( pos & 1 ) ? -offset : offset, comp = pos >> 1;   // comp 0: hor, 1: ver
  const bool use0 = s.refIdx[0] >= 0, use1 = s.refIdx[1] >= 0;
  int        add0 = use0 ? sgn : 0, add1 = use1 ? sgn : 0;   // the offset of each list on component comp
  if( use0 && use1 )
  {
    const int second = mmvdSecondOffset( s.pocDiff[0], s.pocDiff[1], s.longTerm[0] | s.longTerm[1], sgn );
    if( s.pocDiff[0] != s.pocDiff[1] && mmvdCarrier( s.pocDiff[0], s.pocDiff[1] ) == 1 ) add0 = second;
    else add1 = second;
  }
  int interDir = ( use0 ? 1 : 0 ) | ( use1 ? 2 : 0 ), bcw = interDir == 3 ? s.bcwWeightL1 : MMVD_BCW_DEFAULT;
  for( int l = 0; l < 2; l++ )
  {
    if( !( interDir >> l & 1 ) ) continue;
    const int add = l ? add1 : add0;
    out.refIdx[l] = s.refIdx[l];
    out.mv[l][0]  = mmvdStorageClip( s.mv[l][0] + ( comp == 0 ? add : 0 ) );
    out.mv[l][1]  = mmvdStorageClip( s.mv[l][1] + ( comp == 1 ? add : 0 ) );
  }
  if( interDir == 3 && j.width + j.height == 12 )   // restrictBiPredMergeCandsOne
  {
    interDir = 1; out.refIdx[1] = -1; out.mv[1][0] = out.mv[1][1] = 0; bcw = MMVD_BCW_DEFAULT;
  }
  out.interDir = ( uint8_t ) interDir; out.bcwWeightL1 = ( int8_t ) bcw; out.useAltHpelIf = s.useAltHpelIf ? 1 : 0;
  const bool bdof = interDir == 3 && step < MMVD_BDOF_STEPS && mmvdBaseBdof( j, b );
  out.kind = bdof ? VTMHIP_MMVD_BDOF : VTMHIP_MMVD_PLAIN;
  // xCheckIdenticalMotion: both lists name one picture and carry one vector -> xPredInterUni from list 0
  const bool identical = interDir == 3 && s.pocDiff[0] == s.pocDiff[1] && out.mv[0][0] == out.mv[1][0] && out.mv[0][1] == out.mv[1][1];
  predMode = interDir == 3 ? ( identical ? MMVD_PRED_L0 : MMVD_PRED_BI ) : interDir == 2 ? MMVD_PRED_L1 : MMVD_PRED_L0;
  for( int l = 0; l < 2; l++ )
  {
    if( !( predMode == MMVD_PRED_BI || predMode == l ) ) continue;
    predMv[l][0] = mmvdClipAxis( out.mv[l][0], picW, ctuSize, j.posX );
    predMv[l][1] = mmvdClipAxis( out.mv[l][1], picH, ctuSize, j.posY );
  }
}
