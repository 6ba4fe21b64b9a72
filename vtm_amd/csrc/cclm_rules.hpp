// cclm_rules.hpp -- the cross-component linear model (CCLM) rules of the reference's chroma intra prediction for 4:2:0, defined once for host and device: plain
// integer functions without a HIP dependency, so host/test_cclm.cpp compiles them with g++ and the kernels of intra_chroma.hip use the same text.
//   cclmDsSample            IntraPrediction::xGetLumaRecPixels, one down-sampled luma sample           CommonLib/IntraPrediction.cpp:1324-1579
//   cclmTemplate            xGetLMParameters, the template lengths of LM / MDLM_L / MDLM_T             :1672-1688
//   cclmPick                startPos / pickStep / the counts of the up to four template positions      :1689-1730
//   cclmDivSig              the significand table of the division (H.266 8.4.5.2.14)                    :1761-1764
//   cclmParamsFromPairs     the cnt == 2 duplication, the min / max grouping, the division             :1732-1794
//   cclmPredSample          predIntraChromaLM / AreaBuf::linearTransform, one sample                   :268-288
// The regular modes of a chroma block are intra_rules.hpp's with chroma = true.
//
// The down-sampled luma at chroma position (i, j) -- the inner block, the top neighbour row (j = -1) and the left neighbour column (i = -1) -- is ONE function of
// the luma reconstruction plane: its centre is luma (2i, 2j), which puts the top row on luma rows -2 / -1 and the left column on luma columns -3 .. -1 without a
// case of their own.  The reference's two temp buffers (m_piTemp for LM, m_pMdlmTemp for MDLM) are two extents of this one function -- the top row up to W or up
// to W + aboveRight, the left column up to H or up to H + belowLeft -- and are not modelled.
//
// What the host supplies per block (the availability analysis stays host work, as xFillReferenceSamples did for luma): above / left available, the number of
// available above-right / below-left chroma samples (multiples of the chroma unit of 2, at most W / H, zero without above / left), first row of the CTU, the
// collocated flag; the unfiltered Cb and Cr lines top[0 .. 2W], left[0 .. 2H] (index 0 = the corner); and the luma plane around the co-located block, luma (0, 0)
// = the sample under chroma (0, 0): columns 0 .. 2W - 1 of rows 0 .. 2H - 1; with above, rows -3 .. -1 of columns (left ? -3 : 0) .. 2 (W + aboveRight) - 1; with
// left, columns -3 .. -1 of rows (above ? -3 : 0) .. 2 (H + belowLeft) - 1.  host/test_cclm.cpp watches every luma and line index of every (size, availability
// class, mode) through CCLM_LUMA_CHECK / INTRA_LINE_CHECK and finds each inside this.
// Chroma sides are 4, 8, 16, 32.  Side 2 (the chroma of a 4-wide or 4-high luma CU) is not covered: such a block is malformed here.
#pragma once
#include <stdint.h>

#include "intra_rules.hpp"

enum { CCLM_LM = 67, CCLM_MDLM_L = 68, CCLM_MDLM_T = 69, CCLM_NUM_CHROMA_MODE = 70, CCLM_UNIT = 2 };   // CommonDef.h:256-260; the unit: ( 1 << MIN_CU_LOG2 ) >> 1

INTRA_HD bool cclmSideOk( int s ) { return s == 4 || s == 8 || s == 16 || s == 32; }

struct CclmAvail
{
  int above, left;              // 0 / 1
  int aboveRight, belowLeft;    // available chroma samples beyond the block, before the clamp of cclmTemplate
  int firstRow, colocated;      // 0 / 1
};

// what a chroma block must satisfy before anything is read through it
INTRA_HD bool cclmBlockOk( int w, int h, int bitDepth, const CclmAvail &v )
{
  if( !cclmSideOk( w ) || !cclmSideOk( h ) || bitDepth < 8 || bitDepth > 12 ) return false;
  if( ( v.above | v.left | v.firstRow | v.colocated ) & ~1 ) return false;
  if( v.aboveRight < 0 || v.aboveRight > w || ( v.aboveRight & ( CCLM_UNIT - 1 ) ) || ( v.aboveRight && !v.above ) ) return false;
  if( v.belowLeft < 0 || v.belowLeft > h || ( v.belowLeft & ( CCLM_UNIT - 1 ) ) || ( v.belowLeft && !v.left ) ) return false;
  return true;
}
INTRA_HD bool cclmModeOk( int mode ) { return mode >= 0 && mode < CCLM_NUM_CHROMA_MODE; }
INTRA_HD bool cclmIsLm( int mode ) { return mode >= CCLM_LM; }

// every read of the luma plane: CCLM_LUMA_CHECK lets host/test_cclm.cpp see each position before it is used
#ifndef CCLM_LUMA_CHECK
#define CCLM_LUMA_CHECK( x, y )
#endif
struct CclmLuma
{
  const int16_t *p;   // luma (0, 0)
  int            stride;
};
INTRA_HD int cclmLumaAt( const CclmLuma &l, int x, int y )
{
  CCLM_LUMA_CHECK( x, y );
  return l.p[( long ) y * l.stride + x];
}

// i = -1: the left neighbour column (needs left), j = -1: the top neighbour row (needs above); never both
INTRA_HD int cclmDsSample( const CclmLuma &l, const CclmAvail &v, int i, int j )
{
  const int cx = 2 * i, cy = 2 * j;
  const int xl = cx - ( i == 0 && !v.left ? 0 : 1 );   // leftPadding
  if( j < 0 && v.firstRow )                            // one luma row above the CTU boundary: [1 2 1]
    return ( 2 * cclmLumaAt( l, cx, -1 ) + cclmLumaAt( l, xl, -1 ) + cclmLumaAt( l, cx + 1, -1 ) + 2 ) >> 2;
  if( v.colocated )                                    // the cross
  {
    const int yu = cy - ( j == 0 && !v.above ? 0 : 1 );   // abovePadding
    return ( cclmLumaAt( l, cx, yu ) + 4 * cclmLumaAt( l, cx, cy ) + cclmLumaAt( l, xl, cy ) + cclmLumaAt( l, cx + 1, cy ) + cclmLumaAt( l, cx, cy + 1 ) + 4 ) >> 3;
  }
  return ( 2 * cclmLumaAt( l, cx, cy ) + cclmLumaAt( l, cx + 1, cy ) + cclmLumaAt( l, xl, cy ) + 2 * cclmLumaAt( l, cx, cy + 1 ) + cclmLumaAt( l, cx + 1, cy + 1 ) +
           cclmLumaAt( l, xl, cy + 1 ) + 4 ) >> 3;
}

// how far the top row / left column of the down-sampled luma is ever used: the MDLM template lengths
INTRA_HD int cclmTopReach( int w, int h, const CclmAvail &v ) { return v.above ? w + intraMin( v.aboveRight, h ) : 0; }
INTRA_HD int cclmLeftReach( int w, int h, const CclmAvail &v ) { return v.left ? h + intraMin( v.belowLeft, w ) : 0; }

struct CclmTemplate
{
  int above, left;   // the sides the mode uses
  int nTop, nLeft;   // actualTopTemplateSampNum, actualLeftTemplateSampNum
};
INTRA_HD CclmTemplate cclmTemplate( int w, int h, int mode, const CclmAvail &v )
{
  CclmTemplate t = { v.above, v.left, 0, 0 };
  if( mode == CCLM_MDLM_T )
  {
    t.left = 0;
    t.nTop = CCLM_UNIT * ( ( v.above ? w / CCLM_UNIT : 0 ) + intraMin( v.aboveRight / CCLM_UNIT, h / CCLM_UNIT ) );
  }
  else if( mode == CCLM_MDLM_L )
  {
    t.above = 0;
    t.nLeft = CCLM_UNIT * ( ( v.left ? h / CCLM_UNIT : 0 ) + intraMin( v.belowLeft / CCLM_UNIT, w / CCLM_UNIT ) );
  }
  else { t.nTop = w; t.nLeft = h; }
  return t;
}

// the template positions the model is fitted to: the first cntT on the top row, the next cntL on the left column; cntT + cntL is 0, 2 or 4
struct CclmPick
{
  int cntT, startT, stepT, cntL, startL, stepL;
};
INTRA_HD CclmPick cclmPick( const CclmTemplate &t )
{
  const int aboveIs4 = t.left ? 0 : 1, leftIs4 = t.above ? 0 : 1;
  CclmPick  k = { 0, t.nTop >> ( 2 + aboveIs4 ), t.nTop >> ( 1 + aboveIs4 ), 0, t.nLeft >> ( 2 + leftIs4 ), t.nLeft >> ( 1 + leftIs4 ) };
  if( k.stepT < 1 ) k.stepT = 1;
  if( k.stepL < 1 ) k.stepL = 1;
  if( t.above ) k.cntT = intraMin( t.nTop, ( 1 + aboveIs4 ) << 1 );
  if( t.left ) k.cntL = intraMin( t.nLeft, ( 1 + leftIs4 ) << 1 );
  return k;
}

struct CclmModel { int a, b, shift; };

// H.266 8.4.5.2.14 divSigTable: the 4-bit significand of 1 / ( 16 + n ) without its leading bit: round( 256 / ( 16 + n ) ) - 8 for n = 1 .. 15, 0 for n = 0
INTRA_HD int cclmDivSig( int n )
{
  const uint8_t divSigTable[16] = { 0, 7, 6, 5, 5, 4, 4, 3, 3, 2, 2, 1, 1, 1, 1, 0 };
  return divSigTable[n];
}

// the rule from the selected pairs on; cnt: 0 (no neighbour), 2 or 4
INTRA_HD CclmModel cclmParamsFromPairs( const int lumaIn[4], const int chromaIn[4], int cnt, int bitDepth )
{
  CclmModel m = { 0, 1 << ( bitDepth - 1 ), 0 };
  if( cnt == 0 ) return m;
  // cnt == 2: the pairs ( 1, 0, 1, 0 ).  The reference swaps indices into its arrays; the pairs themselves are swapped here (no indexed access: registers)
  int mn0L = lumaIn[cnt == 2 ? 1 : 0], mn0C = chromaIn[cnt == 2 ? 1 : 0], mx0L = lumaIn[cnt == 2 ? 0 : 1], mx0C = chromaIn[cnt == 2 ? 0 : 1];
  int mn1L = lumaIn[cnt == 2 ? 1 : 2], mn1C = chromaIn[cnt == 2 ? 1 : 2], mx1L = lumaIn[cnt == 2 ? 0 : 3], mx1C = chromaIn[cnt == 2 ? 0 : 3], t;
#define CCLM_SWAP( a, b ) { t = a##L; a##L = b##L; b##L = t; t = a##C; a##C = b##C; b##C = t; }
  if( mn0L > mn1L ) CCLM_SWAP( mn0, mn1 )
  if( mx0L > mx1L ) CCLM_SWAP( mx0, mx1 )
  if( mn0L > mx1L ) { CCLM_SWAP( mn0, mx0 ) CCLM_SWAP( mn1, mx1 ) }
  if( mn1L > mx0L ) CCLM_SWAP( mn1, mx0 )
#undef CCLM_SWAP
  const int minL = ( mn0L + mn1L + 1 ) >> 1, minC = ( mn0C + mn1C + 1 ) >> 1;
  const int maxL = ( mx0L + mx1L + 1 ) >> 1, maxC = ( mx0C + mx1C + 1 ) >> 1;
  const int diff = maxL - minL;
  if( diff <= 0 ) { m.b = minC; return m; }
  const int diffC = maxC - minC;
  int       x     = intraLog2( diff );
  const int normDiff = ( ( diff << 4 ) >> x ) & 15;
  const int v = cclmDivSig( normDiff ) | 8;
  x += normDiff != 0;
  const int y   = diffC == 0 ? 0 : intraLog2( intraAbs( diffC ) ) + 1;   // floorLog2( 0 ) = -1
  const int add = ( 1 << y ) >> 1;
  m.a     = ( diffC * v + add ) >> y;
  m.shift = 3 + x - y;
  if( m.shift < 1 )
  {
    m.shift = 1;
    m.a     = m.a == 0 ? 0 : m.a < 0 ? -15 : 15;
  }
  m.b = minC - ( ( m.a * minL ) >> m.shift );
  return m;
}

// the model of one (component, mode): ds( i, j ) = the down-sampled luma (a callable: the closed form itself or a staged copy of it); top / left: the component's lines
template<class Ds>
INTRA_HD CclmModel cclmModel( int w, int h, int mode, int bitDepth, const CclmAvail &v, const int16_t *top, const int16_t *left, const Ds &ds )
{
  const CclmTemplate t = cclmTemplate( w, h, mode, v );
  const CclmPick k = cclmPick( t );
  const int      cnt = k.cntT + k.cntL;
  int luma[4] = { 0, 0, 0, 0 }, chroma[4] = { 0, 0, 0, 0 };
  for( int i = 0; i < 4; i++ )
  {
    if( i < k.cntT )
    {
      const int p = k.startT + i * k.stepT;
      luma[i] = ds( p, -1 ); chroma[i] = intraAt( top, 1 + p, 2 * w );
    }
    else if( i < cnt )
    {
      const int p = k.startL + ( i - k.cntT ) * k.stepL;
      luma[i] = ds( -1, p ); chroma[i] = intraAt( left, 1 + p, 2 * h );
    }
  }
  return cclmParamsFromPairs( luma, chroma, cnt, bitDepth );
}

INTRA_HD int16_t cclmPredSample( const CclmModel &m, int ds, int maxVal ) { return ( int16_t ) intraClip( ( ( m.a * ds ) >> m.shift ) + m.b, maxVal ); }
