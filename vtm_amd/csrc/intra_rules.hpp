// intra_rules.hpp -- the intra prediction rules of the reference for the regular modes (no MIP or BDPCM; luma, and chroma through the `chroma` argument), defined once for host and device: plain integer functions without a HIP
// dependency, so host/test_intra.cpp compiles them with g++ and the kernels of intra.hip use the same text.  ISP builds on them in isp_rules.hpp: the parameters take
// the CU size beside the prediction region's, and the sample rules are templates over the block so that a block with line ends of its own (IspBlk) reads through them.
//   intraWideAngle          IntraPrediction::getModifiedWideAngle                              CommonLib/IntraPrediction.cpp:184-204
//   intraPredParams         IntraPrediction::initPredIntraParams, m_aucIntraFilter             :356-444, :58-68
//   intraFilteredSample     IntraPrediction::xFilterReferenceSamples, one sample of a line     :1166-1200
//   intraDcVal              IntraPrediction::xGetPredValDc                                     :153-182
//   intraPlanarSample       IntraPrediction::xPredIntraPlanar, the row / column sums closed    :294-348
//   intraAngularSample      IntraPrediction::xPredIntraAng, one sample                         :459-643
//   intraPdpcSample         the planar / DC PDPC of predIntraAng                               :244-265
//   intraPredSample         predIntraAng, one sample of the finished prediction                :217-266
//
// The lines: top[0 .. 2W + m] and left[0 .. 2H + m], index 0 of both = the corner sample of reference line m (the reference's buffer with predStride = 2W + 1 + m and
// its second row).  A read of the main line goes through intraLineAt( line, index, last ): an index past `last` reads `last` -- the reference's replication of the last sample of
// the main line (:510-519) by index instead of by a copy.  All other reads go through intraAt unclamped; host/test_intra.cpp watches every index of every
// (shape, mode, m) through INTRA_LINE_CHECK and finds each inside its line.
#pragma once
#include <stdint.h>

#include "../../include/vtmhip.h"

#if defined( __HIPCC__ )
#define INTRA_HD __host__ __device__ inline
#else
#define INTRA_HD inline
#endif

enum { INTRA_PLANAR = 0, INTRA_DC = 1, INTRA_HOR = 18, INTRA_DIA = 34, INTRA_VER = 50, INTRA_VDIA = 66, INTRA_NUM_LUMA_MODE = 67, INTRA_MAX_MRL = 2 };

INTRA_HD int  intraLog2( int v ) { int r = 0; while( ( 2 << r ) <= v ) r++; return r; }   // floorLog2
INTRA_HD bool intraSideOk( int s ) { return s == 4 || s == 8 || s == 16 || s == 32 || s == 64; }
INTRA_HD bool intraIntegerSlope( int absAng ) { return ( absAng & 31 ) == 0; }
INTRA_HD int  intraMin( int a, int b ) { return a < b ? a : b; }
INTRA_HD int  intraAbs( int a ) { return a < 0 ? -a : a; }

// what a block and a job must satisfy before anything is read through them
INTRA_HD bool intraBlockOk( int w, int h, int bitDepth, int m ) { return intraSideOk( w ) && intraSideOk( h ) && bitDepth >= 8 && bitDepth <= 12 && m >= 0 && m <= INTRA_MAX_MRL; }
INTRA_HD bool intraModeOk( int mode, int m ) { return mode >= 0 && mode < INTRA_NUM_LUMA_MODE && !( mode == INTRA_PLANAR && m != 0 ); }

// the mode the angle is taken from: flat blocks trade the modes next to 2 for angles beyond 66 and tall blocks the modes next to 66 for angles below 2
INTRA_HD int intraWideAngle( int w, int h, int mode )
{
  if( mode > INTRA_DC && mode <= INTRA_VDIA )
  {
    const int modeShift[6] = { 0, 6, 10, 12, 14, 15 };
    const int deltaSize    = intraAbs( intraLog2( w ) - intraLog2( h ) );
    if( w > h && mode < 2 + modeShift[deltaSize] ) mode += INTRA_VDIA - 1;
    else if( h > w && mode > INTRA_VDIA - modeShift[deltaSize] ) mode -= INTRA_VDIA - 1;
  }
  return mode;
}

// chroma: a chroma block (m = 0) -- no filter of either kind (:409); everything else, wide angles and PDPC included, from the block's own width and height
// cuW, cuH != 0: w x h is a prediction region of an ISP CU of cuW x cuH (useISP, :361-367, :410) -- the wide-angle shift from the CU, PDPC and angularScale from the
// region, no filter of either kind
INTRA_HD void intraPredParams( int w, int h, int mode, int m, vtmhip_intra_params &p, bool chroma = false, int cuW = 0, int cuH = 0 )
{
  const int angTable[32]    = { 0, 1, 2, 3, 4, 6, 8, 10, 12, 14, 16, 18, 20, 23, 26, 29, 32, 35, 39, 45, 51, 57, 64, 73, 86, 102, 128, 171, 256, 341, 512, 1024 };
  const int invAngTable[32] = { 0,   16384, 8192, 5461, 4096, 2731, 2048, 1638, 1365, 1170, 1024, 910, 819, 712, 630, 565,
                                512, 468,   420,  364,  321,  287,  256,  224,  191,  161,  128,  96,  64,  48,  32,  16 };   // (512 * 32) / angle
  const int mdisThreshold[8] = { 24, 24, 24, 14, 2, 0, 0, 0 };   // by ( log2 W + log2 H ) >> 1
  const int predMode = cuW ? intraWideAngle( cuW, cuH, mode ) : intraWideAngle( w, h, mode );
  const int angMode  = predMode >= INTRA_DIA ? predMode - INTRA_VER : -( predMode - INTRA_HOR );
  p.predMode          = predMode;
  p.isModeVer         = predMode >= INTRA_DIA;
  p.intraPredAngle    = 0;
  p.invAngle          = 0;
  p.angularScale      = 0;
  p.applyPDPC         = w >= 4 && h >= 4 && m == 0;
  p.refFilterFlag     = 0;
  p.interpolationFlag = 0;
  int absAng = 0;
  if( mode > INTRA_DC && mode < INTRA_NUM_LUMA_MODE )
  {
    const int absAngMode = intraAbs( angMode );
    absAng           = angTable[absAngMode];
    p.invAngle       = invAngTable[absAngMode];
    p.intraPredAngle = angMode < 0 ? -absAng : absAng;
    if( angMode < 0 ) p.applyPDPC = 0;
    else if( angMode > 0 )
    {
      const int sideSize = p.isModeVer ? h : w;
      p.angularScale = intraMin( 2, intraLog2( sideSize ) - ( intraLog2( 3 * p.invAngle - 2 ) - 8 ) );
      if( p.angularScale < 0 ) p.applyPDPC = 0;
    }
  }
  if( m != 0 || mode == INTRA_DC || chroma || cuW ) return;
  if( mode == INTRA_PLANAR ) { p.refFilterFlag = w * h > 32; return; }
  const int diff = intraMin( intraAbs( predMode - INTRA_HOR ), intraAbs( predMode - INTRA_VER ) );
  if( diff > mdisThreshold[( intraLog2( w ) + intraLog2( h ) ) >> 1] )
  {
    p.refFilterFlag     = intraIntegerSlope( absAng );   // the [1 2 1] filter on the lines ...
    p.interpolationFlag = !p.refFilterFlag;              // ... or the smoothing taps in the interpolation
  }
}

// every read of a line: INTRA_LINE_CHECK lets host/test_intra.cpp see each index before it is used
#ifndef INTRA_LINE_CHECK
#define INTRA_LINE_CHECK( idx, last )
#endif
INTRA_HD int intraAt( const int16_t *line, int idx, int last )
{
  INTRA_LINE_CHECK( idx, last );
  return line[idx];
}
INTRA_HD int intraLineAt( const int16_t *line, int idx, int last ) { return intraAt( line, idx < last ? idx : last, last ); }

// sample i of a [1 2 1]-filtered line (m = 0): `line` is the line itself of `size` + 1 samples, `other` the other line (the corner takes the first two of both)
INTRA_HD int16_t intraFilteredSample( const int16_t *line, const int16_t *other, int i, int size )
{
  if( i == 0 ) return ( int16_t ) ( ( intraAt( line, 0, size ) + intraAt( line, 1, size ) + other[0] + other[1] + 2 ) >> 2 );
  if( i >= size ) return ( int16_t ) intraAt( line, size, size );
  return ( int16_t ) ( ( intraAt( line, i - 1, size ) + 2 * intraAt( line, i, size ) + intraAt( line, i + 1, size ) + 2 ) >> 2 );
}

// the block as a prediction sees it: the lines it predicts from (filtered where refFilterFlag asks for it)
struct IntraBlk
{
  const int16_t *top, *left;
  int w, h, log2W, log2H, m, maxVal;
};
// the last sample of each line; a block type of its own (isp_rules.hpp's IspBlk) overloads the two
INTRA_HD int intraTopLast( const IntraBlk &b ) { return 2 * b.w + b.m; }
INTRA_HD int intraLeftLast( const IntraBlk &b ) { return 2 * b.h + b.m; }
template<class Blk> INTRA_HD int intraTop( const Blk &b, int i ) { return intraAt( b.top, i, intraTopLast( b ) ); }
template<class Blk> INTRA_HD int intraLeft( const Blk &b, int i ) { return intraAt( b.left, i, intraLeftLast( b ) ); }

template<class Blk> INTRA_HD int16_t intraDcVal( const Blk &b )
{
  const int denom = b.w == b.h ? b.w << 1 : ( b.w > b.h ? b.w : b.h );
  int       sum   = 0;
  if( b.w >= b.h )
    for( int i = 0; i < b.w; i++ ) sum += intraTop( b, b.m + 1 + i );
  if( b.w <= b.h )
    for( int i = 0; i < b.h; i++ ) sum += intraLeft( b, b.m + 1 + i );
  return ( int16_t ) ( ( sum + ( denom >> 1 ) ) >> intraLog2( denom ) );
}

// the row sums of the reference, horPred after x + 1 steps and topRow[x] after y + 1, written out
template<class Blk> INTRA_HD int16_t intraPlanarSample( const Blk &b, int x, int y )
{
  const int top = intraTop( b, x + 1 ), left = intraLeft( b, y + 1 ), topRight = intraTop( b, b.w + 1 ), bottomLeft = intraLeft( b, b.h + 1 );
  const int horPred  = ( left << b.log2W ) + ( x + 1 ) * ( topRight - left );
  const int vertPred = ( top << b.log2H ) + ( y + 1 ) * ( bottomLeft - top );
  return ( int16_t ) ( ( ( horPred << b.log2H ) + ( vertPred << b.log2W ) + ( 1 << ( b.log2W + b.log2H ) ) ) >> ( 1 + b.log2W + b.log2H ) );
}

template<class Blk> INTRA_HD int16_t intraPdpcSample( const Blk &b, int x, int y, int val )
{
  const int scale = ( b.log2W + b.log2H - 2 ) >> 2;
  const int wT = 32 >> intraMin( 31, ( y << 1 ) >> scale ), wL = 32 >> intraMin( 31, ( x << 1 ) >> scale );
  const int left = intraLeft( b, y + 1 ), top = intraTop( b, x + 1 );
  return ( int16_t ) ( val + ( ( wL * ( left - val ) + wT * ( top - val ) + 32 ) >> 6 ) );
}

INTRA_HD int intraClip( int v, int maxVal ) { return v < 0 ? 0 : v > maxVal ? maxVal : v; }

// sample i of the extended main reference (i counted from the corner of line m; negative only for negative angles: the projection of the side line, :489-494)
INTRA_HD int intraRefMain( const int16_t *mainLine, const int16_t *sideLine, int i, int invAngle, int mainLast, int sideSize, int sideLast )
{
  if( i < 0 ) return intraAt( sideLine, intraMin( ( -i * invAngle + 256 ) >> 9, sideSize ), sideLast );
  return intraLineAt( mainLine, i, mainLast );
}

// cubic: the 32 x 4 taps of chroma_taps.hpp.  Horizontal modes are the vertical rule on the transposed block: (r, c) = (row, column) of that block.
// chroma: a fractional slope takes the two-tap rule without a clip (:592-604) and cubic is not read.
template<class Blk> INTRA_HD int16_t intraAngularSample( const vtmhip_intra_params &p, const Blk &b, const int16_t ( *cubic )[4], int x, int y, bool chroma = false )
{
  const bool ver = p.isModeVer != 0;
  const int  r = ver ? y : x, c = ver ? x : y, mainSize = ver ? b.w : b.h, sideSize = ver ? b.h : b.w;
  const int16_t *mainLine = ver ? b.top : b.left, *sideLine = ver ? b.left : b.top;
  const int mainLast = ver ? intraTopLast( b ) : intraLeftLast( b ), sideLast = ver ? intraLeftLast( b ) : intraTopLast( b ), angle = p.intraPredAngle;
  if( angle == 0 )   // pure vertical / horizontal
  {
    int v = intraLineAt( mainLine, b.m + c + 1, mainLast );
    if( p.applyPDPC )
    {
      const int scale = ( b.log2W + b.log2H - 2 ) >> 2;
      if( c < intraMin( 3 << scale, mainSize ) )
      {
        const int wL = 32 >> ( 2 * c >> scale );
        v = intraClip( v + ( ( wL * ( intraAt( sideLine, 1 + r, sideLast ) - intraAt( mainLine, 0, mainLast ) ) + 32 ) >> 6 ), b.maxVal );
      }
    }
    return ( int16_t ) v;
  }
  const int deltaPos = angle * ( r + 1 + b.m ), deltaInt = deltaPos >> 5, deltaFract = deltaPos & 31, i0 = b.m + deltaInt + c;
  int v;
  if( chroma && !intraIntegerSlope( intraAbs( angle ) ) )
  {
    const int p0 = intraRefMain( mainLine, sideLine, i0 + 1, p.invAngle, mainLast, sideSize, sideLast ), p1 = intraRefMain( mainLine, sideLine, i0 + 2, p.invAngle, mainLast, sideSize, sideLast );
    v = ( int16_t ) ( p0 + ( ( deltaFract * ( p1 - p0 ) + 16 ) >> 5 ) );
  }
  else if( !intraIntegerSlope( intraAbs( angle ) ) )
  {
    const int half = deltaFract >> 1;
    int f0, f1, f2, f3;
    if( p.interpolationFlag ) { f0 = 16 - half; f1 = 32 - half; f2 = 16 + half; f3 = half; }
    else { f0 = cubic[deltaFract][0]; f1 = cubic[deltaFract][1]; f2 = cubic[deltaFract][2]; f3 = cubic[deltaFract][3]; }
    const int sum = f0 * intraRefMain( mainLine, sideLine, i0, p.invAngle, mainLast, sideSize, sideLast ) + f1 * intraRefMain( mainLine, sideLine, i0 + 1, p.invAngle, mainLast, sideSize, sideLast ) +
                    f2 * intraRefMain( mainLine, sideLine, i0 + 2, p.invAngle, mainLast, sideSize, sideLast ) + f3 * intraRefMain( mainLine, sideLine, i0 + 3, p.invAngle, mainLast, sideSize, sideLast );
    v = intraClip( ( int16_t ) ( ( sum + 32 ) >> 6 ), b.maxVal );   // through Pel, then the clip
  }
  else v = intraRefMain( mainLine, sideLine, i0 + 1, p.invAngle, mainLast, sideSize, sideLast );
  if( p.applyPDPC && c < intraMin( 3 << p.angularScale, mainSize ) )   // positive angles with m = 0 only
  {
    const int wL   = 32 >> ( 2 * c >> p.angularScale );
    const int left = intraAt( sideLine, r + ( ( 256 + ( c + 1 ) * p.invAngle ) >> 9 ) + 1, sideLast );
    v = ( int16_t ) ( v + ( ( wL * ( left - v ) + 32 ) >> 6 ) );
  }
  return ( int16_t ) v;
}

// b: the lines already chosen by p.refFilterFlag; dcVal: intraDcVal( b ), needed for mode 1 only
template<class Blk> INTRA_HD int16_t intraPredSample( const vtmhip_intra_params &p, int mode, const Blk &b, int dcVal, const int16_t ( *cubic )[4], int x, int y, bool chroma = false )
{
  if( mode > INTRA_DC ) return intraAngularSample( p, b, cubic, x, y, chroma );
  const int v = mode == INTRA_PLANAR ? intraPlanarSample( b, x, y ) : dcVal;
  return p.applyPDPC ? intraPdpcSample( b, x, y, v ) : ( int16_t ) v;
}
