// isp_host.hpp -- the ISP candidate as host arithmetic: what vtmhip_isp_pred_region_host, vtmhip_isp_next_lines_host and vtmhip_isp_chain_host (isp_chain.hip) run, and
// what host/test_isp.cpp compiles with g++ under sanitizers.  No HIP.  The rules are isp_rules.hpp's; the transforms are plain matrix products over
// tr_tables.hpp's matrices and the quantiser is written out here once more, because tu_stages.hpp's is device code -- the device against this text is what
// tests/test_gpu_isp_chain.py checks, and this text against an independent composition what tests/test_isp.py does.  It need not be fast.
//   TrQuant::xT / xIT            CommonLib/TrQuant.cpp:776-923        Quant::quant / dequant, flat list      CommonLib/Quant.cpp:955-1038, 357-482
// Every line a prediction reads is an array of exactly the length the reference's m_topRefLength / m_leftRefLength give it, so an index past a line is an index
// past an allocation.
#pragma once
#include <cstdlib>
#include <vector>

#include "chroma_taps.hpp"
#include "isp_rules.hpp"
#include "tr_tables.hpp"

namespace isp_host
{

inline int clip16( int v ) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }

struct Quant
{
  long long add;
  int       qBits, scale, iscale, rightShift, inMin, inMax;
  Quant( int bitDepth, int qpPer, int qpRem, int isIRAP, int lw, int lh )
  {
    static const int quantScales[2][6]    = { { 26214, 23302, 20560, 18396, 16384, 14564 }, { 18396, 16384, 14564, 13107, 11651, 10280 } };
    static const int invQuantScales[2][6] = { { 40, 45, 51, 57, 64, 72 }, { 57, 64, 72, 80, 90, 102 } };
    const int needSqrt = ( lw + lh ) & 1, trShift = 15 - bitDepth - ( ( lw + lh ) >> 1 ) - needSqrt;
    qBits      = 14 + qpPer + trShift;
    add        = ( long long ) ( isIRAP ? 171 : 85 ) << ( qBits - 9 );
    scale      = quantScales[needSqrt][qpRem];
    iscale     = invQuantScales[needSqrt][qpRem];
    rightShift = 6 - ( trShift + qpPer );
    const int inBits = 32 + rightShift - 7 < 16 ? 32 + rightShift - 7 : 16;
    inMin = -( 1 << ( inBits - 1 ) );
    inMax = ( 1 << ( inBits - 1 ) ) - 1;
  }
  int level( int c, long long &absSum ) const
  {
    const int m = ( int ) ( ( ( long long ) std::abs( c ) * scale + add ) >> qBits );
    absSum += m;
    return clip16( c < 0 ? -m : m );
  }
  int dequant( int q ) const
  {
    const int qq = q < inMin ? inMin : q > inMax ? inMax : q;
    if( rightShift > 0 ) return clip16( ( int ) ( ( unsigned ) ( qq * iscale ) + ( 1u << ( rightShift - 1 ) ) ) >> rightShift );
    return clip16( ( int ) ( ( unsigned ) ( qq * iscale ) << ( -rightShift ) ) );
  }
};

// dst[k * dstLd + j] = (sum_n M[k][n] * src[j * srcLd + n] + rnd) >> shift for j < lines, k < N; zero for j >= linesEff or k >= kEff
inline void fwdPass( const int *src, int srcLd, int *dst, int dstLd, const int16_t *M, int N, int lines, int linesEff, int kEff, int shift )
{
  const unsigned rnd = shift > 0 ? 1u << ( shift - 1 ) : 0;
  for( int j = 0; j < lines; j++ )
    for( int k = 0; k < N; k++ )
    {
      unsigned sum = 0;
      if( j < linesEff && k < kEff )
        for( int n = 0; n < N; n++ ) sum += ( unsigned ) src[j * srcLd + n] * ( unsigned ) ( int ) M[k * N + n];
      dst[k * dstLd + j] = ( j < linesEff && k < kEff ) ? ( int ) ( sum + rnd ) >> shift : 0;
    }
}

// dst[i * N + j] = clip16( (sum_{k < cut} src[k * srcLd + i] * M[k][j] + rnd) >> shift ) for i < lines, j < N; zero for i >= linesEff
inline void invPass( const int *src, int srcLd, int *dst, const int16_t *M, int N, int lines, int linesEff, int cut, int shift )
{
  const unsigned rnd = 1u << ( shift - 1 );
  for( int i = 0; i < lines; i++ )
    for( int j = 0; j < N; j++ )
    {
      unsigned sum = 0;
      for( int k = 0; k < cut && i < linesEff; k++ ) sum += ( unsigned ) src[k * srcLd + i] * ( unsigned ) ( int ) M[k * N + j];
      dst[i * N + j] = i < linesEff ? clip16( ( int ) ( sum + rnd ) >> shift ) : 0;
    }
}

inline std::vector<int16_t> matrix( int type, int n )
{
  std::vector<int16_t> m( ( size_t ) n * n );
  if( n > 1 ) vtmhip_tr_matrix( type, n, m.data() );
  return m;
}

// one TU: resi (w x h, row-major) -> levels (the same shape), the reconstructed residual, sum |coefficient| and sum |level|
inline void tuChain( const int *resi, int w, int h, int bitDepth, int qpPer, int qpRem, int isIRAP, int *levels, int *rec, long long &sumAbs, long long &absSum )
{
  const int lw = intraLog2( w ), lh = intraLog2( h ), skipW = ispTrSkip( w ), skipH = ispTrSkip( h );
  const std::vector<int16_t> mw = matrix( ispTrType( w ), w ), mh = matrix( ispTrType( h ), h );
  std::vector<int> tmp( ( size_t ) w * h ), coef( ( size_t ) w * h );
  if( w > 1 && h > 1 )
  {
    fwdPass( resi, w, tmp.data(), h, mw.data(), w, h, h, w - skipW, ispFwdShift1( lw, bitDepth ) );
    fwdPass( tmp.data(), h, coef.data(), w, mh.data(), h, w, w - skipW, h - skipH, ispFwdShift2( lh ) );
  }
  else if( h == 1 ) fwdPass( resi, w, coef.data(), 1, mw.data(), w, 1, 1, w - skipW, ispFwdShift1( lw, bitDepth ) );
  else fwdPass( resi, h, coef.data(), 1, mh.data(), h, 1, 1, h - skipH, ispFwdShift1( lh, bitDepth ) );
  const Quant q( bitDepth, qpPer, qpRem, isIRAP, lw, lh );
  for( int i = 0; i < w * h; i++ )
  {
    sumAbs += std::abs( coef[i] );
    levels[i] = q.level( coef[i], absSum );
    coef[i]   = q.dequant( levels[i] );
  }
  if( w > 1 && h > 1 )
  {
    invPass( coef.data(), w, tmp.data(), mh.data(), h, w, w - skipW, h - skipH, ispInvShift1() );
    invPass( tmp.data(), h, rec, mw.data(), w, h, h, w - skipW, ispInvShift2( bitDepth ) );
  }
  else if( h == 1 ) invPass( coef.data(), 1, rec, mw.data(), w, 1, 1, w - skipW, ispInvShift1D( bitDepth ) );
  else invPass( coef.data(), 1, rec, mh.data(), h, 1, 1, h - skipH, ispInvShift1D( bitDepth ) );
}

// predIntraAng of a regW x regH region of a cuW x cuH CU from lines of exactly cuW + regW + 1 and cuH + regH + 1 samples; pred at predStride
inline void predRegion( int cuW, int cuH, int regW, int regH, int mode, int bitDepth, const int16_t *top, const int16_t *left, int16_t *pred, int predStride )
{
  static const int16_t cubic[32][4] = { VTMHIP_CHROMA_FILTER_TAPS };
  vtmhip_intra_params p;
  ispPredParams( cuW, cuH, regW, regH, mode, p );
  IspBlk b;
  b.top = top; b.left = left; b.w = regW; b.h = regH; b.log2W = intraLog2( regW ); b.log2H = intraLog2( regH ); b.m = 0; b.maxVal = ( 1 << bitDepth ) - 1;
  b.topLast = cuW + regW; b.leftLast = cuH + regH;
  const int dc = mode == INTRA_DC ? intraDcVal( b ) : 0;
  for( int y = 0; y < regH; y++ )
    for( int x = 0; x < regW; x++ ) pred[y * predStride + x] = intraPredSample( p, mode, b, dc, cubic, x, y );
}

// the lines region r >= 1 sees: topOut[0 .. cuW + regW], leftOut[0 .. cuH + regH]
inline void nextLines( const IspLines &l, const IspGeom &g, int cuW, int cuH, int r, int16_t *topOut, int16_t *leftOut )
{
  int16_t  *mainOut = l.split == ISP_HOR ? topOut : leftOut, *sideOut = l.split == ISP_HOR ? leftOut : topOut;
  const int mainLast = l.split == ISP_HOR ? cuW + g.regW : cuH + g.regH, sideLast = l.split == ISP_HOR ? cuH + g.regH : cuW + g.regW;
  for( int i = 0; i <= mainLast; i++ ) mainOut[i] = ( int16_t ) ispMainAt( l, g, r, i );
  for( int i = 0; i <= sideLast; i++ ) sideOut[i] = ( int16_t ) ispSideAt( l, g, r, i );
}

// one candidate; the tables have passed ispScan
inline void chainJob( const int16_t *refBase, const int16_t *orgBase, const vtmhip_intra_block &B, const vtmhip_isp_job &J, int16_t *predBase, int32_t *levelsBase,
                      int16_t *recoBase, vtmhip_isp_result &res )
{
  const int W = B.width, H = B.height, bd = B.bitDepth, maxVal = ( 1 << bd ) - 1;
  IspGeom   g;
  ispGeometry( W, H, J.split, g );
  const int16_t *cuTop = refBase + B.refOff, *cuLeft = cuTop + 2 * W + 1, *org = orgBase + B.orgOff;
  std::vector<int16_t> reco( ( size_t ) W * H ), top( ( size_t ) W + g.regW + 1 ), left( ( size_t ) H + g.regH + 1 );
  const IspLines lines = { cuTop, cuLeft, reco.data(), W, J.split, J.sideAvail };
  res = vtmhip_isp_result();
  res.numParts = g.numParts;
  for( int r = 0; r < g.numRegions; r++ )
  {
    const int rx = J.split == ISP_HOR ? 0 : r * g.ext, ry = J.split == ISP_HOR ? r * g.ext : 0;
    if( r == 0 )
    {
      for( size_t i = 0; i < top.size(); i++ ) top[i] = cuTop[i];
      for( size_t i = 0; i < left.size(); i++ ) left[i] = cuLeft[i];
    }
    else nextLines( lines, g, W, H, r, top.data(), left.data() );
    predRegion( W, H, g.regW, g.regH, J.mode, bd, top.data(), left.data(), reco.data() + ry * W + rx, W );   // the prediction lies where the reconstruction will
    if( predBase )
      for( int y = 0; y < g.regH; y++ )
        for( int x = 0; x < g.regW; x++ ) predBase[J.predOff + ( ry + y ) * W + rx + x] = reco[( ry + y ) * W + rx + x];
    for( int q = 0; q < g.tusPerRegion; q++ )
    {
      const int k = r * g.tusPerRegion + q, pw = g.partW, ph = g.partH;
      int       px, py;
      ispPartRect( g, J.split, k, px, py );
      std::vector<int> resi( ( size_t ) pw * ph ), levels( ( size_t ) pw * ph ), rec( ( size_t ) pw * ph );
      for( int y = 0; y < ph; y++ )
        for( int x = 0; x < pw; x++ ) resi[y * pw + x] = org[( long ) ( py + y ) * B.orgStride + px + x] - reco[( py + y ) * W + px + x];
      long long sumAbs = 0, absSum = 0;
      tuChain( resi.data(), pw, ph, bd, J.qpPer, J.qpRem, J.isIRAP, levels.data(), rec.data(), sumAbs, absSum );
      uint64_t sse = 0;
      for( int y = 0; y < ph; y++ )
        for( int x = 0; x < pw; x++ )
        {
          const int v = intraClip( reco[( py + y ) * W + px + x] + rec[y * pw + x], maxVal ), d = org[( long ) ( py + y ) * B.orgStride + px + x] - v;
          reco[( py + y ) * W + px + x] = ( int16_t ) v;
          sse += ( uint64_t ) ( ( unsigned ) d * ( unsigned ) d );
          if( levelsBase ) levelsBase[J.outOff + ( long ) k * pw * ph + y * pw + x] = levels[y * pw + x];
        }
      res.sse[k] = sse; res.absSum[k] = ( int32_t ) absSum; res.sumAbs[k] = ( int32_t ) sumAbs;
    }
  }
  for( int i = 0; i < W * H; i++ ) recoBase[J.outOff + i] = reco[i];
}

}   // namespace isp_host
