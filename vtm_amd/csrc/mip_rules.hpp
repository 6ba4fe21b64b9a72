// mip_rules.hpp -- the matrix-based intra prediction (MIP) rules of the reference for a luma block, defined once for host and device: plain integer functions without
// a HIP dependency, so host/test_mip.cpp compiles them with g++ and the kernel of mip.hip uses the same text.
//   mipSizeId, mipNumModes   getMipSizeId, getNumModesMip                                       CommonLib/UnitTools.cpp:3873-3900
//   mipShape                 MatrixIntraPrediction::initPredBlockParams                         CommonLib/MatrixIntraPrediction.cpp:140-159
//   mipBoundarySample        boundaryDownsampling1D, one entry                                  :163-191
//   mipInputAt               the two input orders and the rebasing of prepareInputForPred       :94-117
//   mipReducedSample         computeReducedPred, one entry (mipRedIndex: its transposition)     :283-335
//   mipSample                predictionUpsampling / predictionUpsampling1D, one output sample   :194-267
//
// The lines are those of a vtmhip_intra_block on reference line 0: top[0 .. 2W] and left[0 .. 2H] with index 0 = the corner.  MIP reads top[1 .. W] and left[1 .. H]
// and nothing else; every read goes through mipAt, and host/test_mip.cpp watches each index through MIP_LINE_CHECK.
//
// Up-sampling as a closed form.  The reference interpolates horizontally first, on the anchor rows (r + 1) * upV - 1 only and with left[] at those rows as the sample
// before column 0, then vertically between anchor rows with top[] as the row before row 0; each 1-D pass rounds.  With c = x / upH, px = x % upH + 1, k = y / upV,
// py = y % upV + 1:
//   H( r, x ) = ( ( upH - px ) * ( c ? red[r][c - 1] : left[( r + 1 ) * upV - 1] ) + px * red[r][c] + upH / 2 ) >> log2 upH
//   out       = ( ( upV - py ) * ( k ? H( k - 1, x ) : top[x] ) + py * H( k, x ) + upV / 2 ) >> log2 upV
// (0-based neighbour samples: left[j] here is line index j + 1).  A factor of 1 is the identity.
#pragma once
#include <stdint.h>

#if defined( __HIPCC__ )
#define MIP_HD __host__ __device__ inline
#else
#define MIP_HD inline
#endif

enum
{
  MIP_SHIFT_MATRIX = 6, MIP_OFFSET_MATRIX = 32, MIP_MAX_INPUT = 8, MIP_MAX_REDUCED = 64,
  MIP_BYTES_4X4 = 16 * 16 * 4, MIP_BYTES_8X8 = 8 * 16 * 8, MIP_BYTES_16X16 = 6 * 64 * 7   // mipMatrix4x4 / 8x8 / 16x16 of MipData.h
};

MIP_HD int  mipLog2( int v ) { int r = 0; while( ( 2 << r ) <= v ) r++; return r; }   // floorLog2
MIP_HD bool mipSideOk( int s ) { return s == 4 || s == 8 || s == 16 || s == 32 || s == 64; }
MIP_HD int  mipSizeId( int w, int h ) { return w == 4 && h == 4 ? 0 : ( w == 4 || h == 4 || ( w == 8 && h == 8 ) ) ? 1 : 2; }
MIP_HD int  mipNumModes( int sizeId ) { return sizeId == 0 ? 16 : sizeId == 1 ? 8 : 6; }

struct MipShape
{
  int w, h, sizeId;
  int bdry;   // entries of one reduced boundary: 2 / 4
  int pred;   // side of the reduced prediction: 4 / 8
  int upH, upV, log2UpH, log2UpV;
};

MIP_HD MipShape mipShape( int w, int h )
{
  MipShape s;
  s.w = w; s.h = h; s.sizeId = mipSizeId( w, h );
  s.bdry = s.sizeId == 0 ? 2 : 4;
  s.pred = s.sizeId < 2 ? 4 : 8;
  s.upH = w / s.pred; s.upV = h / s.pred;
  s.log2UpH = mipLog2( s.upH ); s.log2UpV = mipLog2( s.upV );
  return s;
}

// what a block and a job must satisfy before anything is read through them
MIP_HD bool mipBlockOk( int w, int h, int bitDepth, int multiRefIdx ) { return mipSideOk( w ) && mipSideOk( h ) && bitDepth >= 8 && bitDepth <= 12 && multiRefIdx == 0; }
MIP_HD bool mipJobOk( const MipShape &s, int mode, int transposed ) { return mode >= 0 && mode < mipNumModes( s.sizeId ) && transposed >= 0 && transposed <= 1; }

// the weights of one mode: [pred * pred][4 / 8 / 7] bytes; size id 2 has no column for the first input
MIP_HD int mipMatrixCols( int sizeId ) { return sizeId == 0 ? 4 : sizeId == 1 ? 8 : 7; }
MIP_HD const uint8_t *mipMatrix( const MipShape &s, int mode, const uint8_t *m4x4, const uint8_t *m8x8, const uint8_t *m16x16 )
{
  return ( s.sizeId == 0 ? m4x4 : s.sizeId == 1 ? m8x8 : m16x16 ) + mode * s.pred * s.pred * mipMatrixCols( s.sizeId );
}

// every read of a line: MIP_LINE_CHECK lets host/test_mip.cpp see each index before it is used (valid: 1 .. last)
#ifndef MIP_LINE_CHECK
#define MIP_LINE_CHECK( idx, last )
#endif
MIP_HD int mipAt( const int16_t *line, int idx, int last )
{
  MIP_LINE_CHECK( idx, last );
  return line[idx];
}

// entry i of the reduced boundary of a line of `len` samples (line[1 .. len]): the rounded mean of len / bdry neighbours, or the sample itself
MIP_HD int mipBoundarySample( const int16_t *line, int len, int bdry, int i )
{
  if( bdry >= len ) return mipAt( line, 1 + i, len );
  const int f = len / bdry, log2F = mipLog2( f );
  int sum = 0;
  for( int k = 0; k < f; k++ ) sum += mipAt( line, 1 + i * f + k, len );
  return ( sum + ( 1 << ( log2F - 1 ) ) ) >> log2F;
}

// entry i of the rebased input whose first half is the reduced boundary `a` and whose second half is `b` (top | left, or left | top for transposed); the input
// offset of that order is a[0]
MIP_HD int mipInputAt( const MipShape &s, int bitDepth, const int *a, const int *b, int i )
{
  if( i == 0 ) return s.sizeId < 2 ? ( 1 << ( bitDepth - 1 ) ) - a[0] : 0;
  return ( i < s.bdry ? a[i] : b[i - s.bdry] ) - a[0];
}

// entry `pos` (row-major, before the transposition) of the reduced prediction; `matrix`: mipMatrix() of the mode
MIP_HD int mipReducedSample( const MipShape &s, const int *in, int inputOffset, int bitDepth, const uint8_t *matrix, int pos )
{
  const int n = 2 * s.bdry, cols = mipMatrixCols( s.sizeId ), skip = n - cols;   // skip 1: the first input has no weight (and is 0)
  const uint8_t *weight = matrix + pos * cols;
  int sum = 0, acc = 0;
  for( int i = 0; i < n; i++ ) sum += in[i];
  for( int i = skip; i < n; i++ ) acc += in[i] * weight[i - skip];
  const int v = ( ( acc + ( 1 << ( MIP_SHIFT_MATRIX - 1 ) ) - MIP_OFFSET_MATRIX * sum ) >> MIP_SHIFT_MATRIX ) + inputOffset, maxVal = ( 1 << bitDepth ) - 1;
  return v < 0 ? 0 : v > maxVal ? maxVal : v;
}
// where entry `pos` lands in the reduced block red[pred][pred]
MIP_HD int mipRedIndex( const MipShape &s, int transposed, int pos ) { return transposed ? ( pos % s.pred ) * s.pred + pos / s.pred : pos; }

// the horizontally interpolated sample of anchor row r (reduced row r) at column x
MIP_HD int mipHorSample( const MipShape &s, const int16_t *red, const int16_t *left, int r, int x )
{
  if( s.upH == 1 ) return red[r * s.pred + x];
  const int c = x >> s.log2UpH, px = ( x & ( s.upH - 1 ) ) + 1;
  const int before = c ? red[r * s.pred + c - 1] : mipAt( left, ( r + 1 ) * s.upV, s.h );
  return ( ( s.upH - px ) * before + px * red[r * s.pred + c] + ( s.upH >> 1 ) ) >> s.log2UpH;
}

// sample (x, y) of the finished W x H prediction from the reduced block (already transposed where asked for)
MIP_HD int16_t mipSample( const MipShape &s, const int16_t *red, const int16_t *top, const int16_t *left, int x, int y )
{
  if( s.upV == 1 ) return ( int16_t ) mipHorSample( s, red, left, y, x );
  const int k = y >> s.log2UpV, py = ( y & ( s.upV - 1 ) ) + 1;
  const int behind = mipHorSample( s, red, left, k, x );
  if( py == s.upV ) return ( int16_t ) behind;   // an anchor row
  const int before = k ? mipHorSample( s, red, left, k - 1, x ) : mipAt( top, x + 1, s.w );
  return ( int16_t ) ( ( ( s.upV - py ) * before + py * behind + ( s.upV >> 1 ) ) >> s.log2UpV );
}

// the whole prediction on the host (vtmhip_mip_pred_host, host/test_mip.cpp): pred[H][W], stride W
MIP_HD void mipPredict( int w, int h, int bitDepth, int mode, int transposed, const int16_t *top, const int16_t *left, const uint8_t *m4x4, const uint8_t *m8x8,
                        const uint8_t *m16x16, int16_t *pred )
{
  const MipShape s = mipShape( w, h );
  int redTop[4], redLeft[4], in[MIP_MAX_INPUT];
  for( int i = 0; i < s.bdry; i++ )
  {
    redTop[i]  = mipBoundarySample( top, w, s.bdry, i );
    redLeft[i] = mipBoundarySample( left, h, s.bdry, i );
  }
  const int *a = transposed ? redLeft : redTop, *b = transposed ? redTop : redLeft;
  for( int i = 0; i < 2 * s.bdry; i++ ) in[i] = mipInputAt( s, bitDepth, a, b, i );
  const uint8_t *matrix = mipMatrix( s, mode, m4x4, m8x8, m16x16 );
  int16_t red[MIP_MAX_REDUCED];
  for( int pos = 0; pos < s.pred * s.pred; pos++ ) red[mipRedIndex( s, transposed, pos )] = ( int16_t ) mipReducedSample( s, in, a[0], bitDepth, matrix, pos );
  for( int y = 0; y < h; y++ )
    for( int x = 0; x < w; x++ ) pred[y * w + x] = mipSample( s, red, top, left, x, y );
}
