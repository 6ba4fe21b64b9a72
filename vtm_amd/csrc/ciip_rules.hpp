// ciip_rules.hpp -- the rules of combined inter-intra prediction (CIIP) of the reference, defined once for host and device: plain integer functions without a HIP
// dependency, so host/test_ciip.cpp compiles them with g++ and the kernels of ciip.hip use the same text.
//   ciipSizeOk            the eligibility of a CU: w * h >= 64, w < 128, h < 128                              EncoderLib/EncCu.cpp:2335-2339
//   ciipNumCand           how many entries of RdModeList the CIIP loop tests                                  :2471
//   ciipWeightIntra       the neighbour rule of IntraPrediction::geneWeightedPred                             CommonLib/IntraPrediction.cpp:693-714
//   ciipBlendSample       its sample rule, without a clip                                                     :719
//   ciipLutAt             PelBuf::rspSignal, one sample (the index held inside the table)                     CommonLib/Buffer.h
//   ciipIntraParams / ciipIntraSample   the intra part: planar with multiRefIdx 0 under the regular rules -- intra_rules.hpp's intraPredParams (refFilterFlag =
//                         w * h > 32 for luma, none for chroma; PDPC on) and intraPredSample, unchanged
//   ciipLineSample        one sample of the lines a block predicts from: the [1 2 1] filter (intraFilteredSample) where refFilterFlag asks for it
//   ciipCandOk / ciipJobOk / ciipBlendJobOk   what a row of the two device tables must satisfy before anything is read through it
//   ciipHostIntra / ciipHostBlend   a whole block on the host: vtmhip_ciip_host and vtmhip_ciip_blend_host are these
#pragma once
#include <stdint.h>

#include "intra_rules.hpp"

#define CIIP_HD INTRA_HD

enum { CIIP_NUM_MRG_SATD_CAND = 4, CIIP_MODE_L0 = 0, CIIP_MODE_L1 = 1, CIIP_MODE_BI = 2, CIIP_MODE_GIVEN = 3 };
enum { CIIP_LINE = 136 };   // 2 * 64 + 1 samples of a line, rounded up to a multiple of 8

CIIP_HD bool ciipSizeOk( int w, int h ) { return intraSideOk( w ) && intraSideOk( h ) && w * h >= 64; }   // sides are powers of two from 4: < 128 is <= 64
// the 4:2:0 chroma block of a CIIP CU: a width of 2 stays unblended (EncCu.cpp:2718), a height of 2 (16x4, 32x4, 64x4 luma) is blended, without PDPC
CIIP_HD bool ciipChromaSizeOk( int w, int h )
{
  return ( w == 4 || w == 8 || w == 16 || w == 32 ) && ( h == 2 || h == 4 || h == 8 || h == 16 || h == 32 ) && w * h >= 16;
}
CIIP_HD int  ciipNumCand( int numValidMergeCand )
{
  const int n = numValidMergeCand < CIIP_NUM_MRG_SATD_CAND ? numValidMergeCand : CIIP_NUM_MRG_SATD_CAND;
  return n < 0 ? 0 : n < 4 ? n : 4;
}

CIIP_HD int ciipWeightIntra( int leftIntra, int aboveIntra ) { return 1 + ( leftIntra != 0 ) + ( aboveIntra != 0 ); }
CIIP_HD int ciipBlendSample( int inter, int intra, int wIntra ) { return ( ( 4 - wIntra ) * inter + wIntra * intra + 2 ) >> 2; }
CIIP_HD int ciipLutAt( const int16_t *lut, int v, int maxVal ) { return lut[v < 0 ? 0 : v > maxVal ? maxVal : v]; }

CIIP_HD void ciipIntraParams( int w, int h, bool chroma, vtmhip_intra_params &p ) { intraPredParams( w, h, INTRA_PLANAR, 0, p, chroma ); }
CIIP_HD IntraBlk ciipIntraBlk( const int16_t *top, const int16_t *left, int w, int h, int bitDepth )
{
  IntraBlk b;
  b.top = top; b.left = left; b.w = w; b.h = h; b.log2W = intraLog2( w ); b.log2H = intraLog2( h ); b.m = 0; b.maxVal = ( 1 << bitDepth ) - 1;
  return b;
}
// b: the lines p.refFilterFlag chooses
CIIP_HD int ciipIntraSample( const vtmhip_intra_params &p, const IntraBlk &b, int x, int y, bool chroma )
{
  return intraPredSample( p, INTRA_PLANAR, b, 0, ( const int16_t( * )[4] ) nullptr, x, y, chroma );
}

// sample i of the lines a block predicts from: top at [0, 2w], left at [2w + 1, 2w + 2h + 1] of `lines`; filtered != 0: through the [1 2 1] filter
CIIP_HD int16_t ciipLineSample( const int16_t *lines, int w, int h, int i, int filtered )
{
  const int      nTop = 2 * w + 1;
  const int16_t *top = lines, *left = lines + nTop;
  if( !filtered ) return lines[i];
  return i < nTop ? intraFilteredSample( top, left, i, 2 * w ) : intraFilteredSample( left, top, i - nTop, 2 * h );
}

CIIP_HD bool ciipCandOk( const vtmhip_ciip_cand &c, int w )
{
  if( c.mode > CIIP_MODE_GIVEN ) return false;
  if( c.mode == CIIP_MODE_GIVEN ) return c.srcStride >= w;
  if( c.mode != CIIP_MODE_L1 && c.refStride[0] < w ) return false;
  if( c.mode != CIIP_MODE_L0 && c.refStride[1] < w ) return false;
  return true;
}

// callLmcs: 0, or the depth of the context's two LUTs in a call that allows LMCS jobs
CIIP_HD bool ciipJobOk( const vtmhip_ciip_job &j, int maxW, int maxH, int callLmcs )
{
  if( !ciipSizeOk( j.width, j.height ) || j.width > maxW || j.height > maxH || j.bitDepth < 8 || j.bitDepth > 12 ) return false;
  if( j.numCand < 1 || j.numCand > 4 || j.orgStride < j.width ) return false;
  if( j.lmcs && callLmcs != j.bitDepth ) return false;
  for( int k = 0; k < j.numCand; k++ )
    if( !ciipCandOk( j.cand[k], j.width ) ) return false;
  return true;
}

// fwdDepth: 0, or the depth of the forward LUT the call can reach
CIIP_HD bool ciipBlendJobOk( const vtmhip_ciip_blend_job &j, int fwdDepth )
{
  if( j.bitDepth < 8 || j.bitDepth > 12 || j.predStride < j.width ) return false;
  if( j.chroma ) return ciipChromaSizeOk( j.width, j.height ) && !j.mapFwd;
  return ciipSizeOk( j.width, j.height ) && ( !j.mapFwd || fwdDepth == j.bitDepth );
}

// ---- whole blocks on the host ---------------------------------------------------------------------------------------------------------------------------------
// lines: top (2w + 1), then left (2h + 1); intra: w x h, stride w
inline void ciipHostIntra( const int16_t *lines, int w, int h, int bitDepth, bool chroma, int16_t *intra )
{
  vtmhip_intra_params p;
  ciipIntraParams( w, h, chroma, p );
  int16_t   used[2 * CIIP_LINE];
  const int n = 2 * w + 1 + 2 * h + 1;
  for( int i = 0; i < n; i++ ) used[i] = ciipLineSample( lines, w, h, i, p.refFilterFlag );
  const IntraBlk b = ciipIntraBlk( used, used + 2 * w + 1, w, h, bitDepth );
  for( int y = 0; y < h; y++ )
    for( int x = 0; x < w; x++ ) intra[y * w + x] = ( int16_t ) ciipIntraSample( p, b, x, y, chroma );
}

// geneWeightedPred over the inter block at pred, in place; fwdLut != nullptr: the inter block goes through it first
inline void ciipHostBlend( int16_t *pred, int predStride, const int16_t *intra, int w, int h, int bitDepth, int wIntra, const int16_t *fwdLut )
{
  for( int y = 0; y < h; y++ )
    for( int x = 0; x < w; x++ )
    {
      int v = pred[y * predStride + x];
      if( fwdLut ) v = ciipLutAt( fwdLut, v, ( 1 << bitDepth ) - 1 );
      pred[y * predStride + x] = ( int16_t ) ciipBlendSample( v, intra[y * w + x], wIntra );
    }
}
