// intra_body.hpp -- the workgroup body of the intra luma kernels that work from a vtmhip_intra_block table, shared by intra.hip (intra_kernel: the prediction alone, or
// kept in LDS and reduced to SAD and SATD) and intra_chain.hip (intra_resi_kernel: prediction and residual).  How a workgroup walks its jobs is described in intra.hip.
#pragma once
#include "ctx.hpp"
#include "chroma_taps.hpp"
#include "dist_block.hpp"
#include "intra_lane_rule.hpp"
#include "intra_rules.hpp"

namespace
{

__constant__ int16_t c_intraCubic[32][4] = { VTMHIP_CHROMA_FILTER_TAPS };   // InterpolationFilter::getChromaFilterTable (IntraPrediction.cpp:576)

constexpr int INTRA_LINE = 136;    // 2 * 64 + 1 + 2 samples of a line, rounded up

struct IntraLds
{
  int16_t *line;   // [4][INTRA_LINE]: top, left, filtered top, filtered left
  int     *dc;
  int16_t *org, *pred;   // org: fused and residual modes; pred: fused only
};

// what a job leaves behind: its prediction in global memory; SAD and SATD of the prediction kept in LDS; prediction and residual (original - prediction) in global memory
enum IntraOut { INTRA_OUT_PRED, INTRA_OUT_DIST, INTRA_OUT_RESI };

template<int L, IntraOut OUT>
__device__ __forceinline__ void intra_chunk_body( const IntraLds &s, const int16_t *__restrict__ refBase, const int16_t *__restrict__ orgBase,
                                                  const vtmhip_intra_block *__restrict__ blocks, int numBlocks, const vtmhip_intra_job *__restrict__ jobs, int n,
                                                  int16_t *__restrict__ predBase, unsigned long long *__restrict__ dist, int16_t *__restrict__ resiBase = nullptr )
{
  constexpr bool FUSED = OUT == INTRA_OUT_DIST, RESI = OUT == INTRA_OUT_RESI;
  constexpr int G = 256 / L, CHUNK = L == 16 ? 16 : L == 64 ? 8 : 4;
  const int tid = threadIdx.x, g = tid / L, l = tid % L;
  const int jBegin = blockIdx.x * CHUNK, jEnd = min( n, jBegin + CHUNK );
  int16_t  *sTop = s.line, *sLeft = s.line + INTRA_LINE, *sFTop = s.line + 2 * INTRA_LINE, *sFLeft = s.line + 3 * INTRA_LINE;

  for( int j = jBegin; j < jEnd; )
  {
    // the run [j, e) of one block index (uniform over the workgroup)
    const int blk = uni( jobs[j].block );
    int       e   = j + 1;
    while( e < jEnd && uni( jobs[e].block ) == blk ) e++;
    const int first = j;
    j = e;
    if( blk < 0 || blk >= numBlocks ) continue;
    const vtmhip_intra_block B = blocks[blk];
    const int w = uni( ( int ) B.width ), h = uni( ( int ) B.height ), m = uni( ( int ) B.multiRefIdx ), bd = uni( ( int ) B.bitDepth );
    if( !intraBlockOk( w, h, bd, m ) || w * h > ( L == 16 ? 64 : L == 64 ? 1024 : INTRA_MAX_AREA ) ) continue;   // the second part cannot happen: L comes from the largest block
    const int area = w * h, log2W = intraLog2( w ), log2H = intraLog2( h ), nTop = 2 * w + 1 + m, nLeft = 2 * h + 1 + m;

    __syncthreads();   // the previous run's readers are done
    {
      const int16_t *ref = refBase + B.refOff;
      for( int i = tid; i < nTop + nLeft; i += 256 )
      {
        const int16_t v = ref[i];
        if( i < nTop ) sTop[i] = v;
        else sLeft[i - nTop] = v;
      }
      if( FUSED || RESI )
      {
        const int16_t *org = orgBase + B.orgOff;
        for( int i = tid; i < area; i += 256 ) s.org[i] = org[( long ) ( i >> log2W ) * B.orgStride + ( i & ( w - 1 ) )];
      }
    }
    __syncthreads();
    if( m == 0 )   // the filtered lines exist for m = 0 only (refFilterFlag)
      for( int i = tid; i < nTop + nLeft; i += 256 )
      {
        if( i < nTop ) sFTop[i] = intraFilteredSample( sTop, sLeft, i, 2 * w );
        else sFLeft[i - nTop] = intraFilteredSample( sLeft, sTop, i - nTop, 2 * h );
      }
    IntraBlk U;
    U.top = sTop; U.left = sLeft; U.w = w; U.h = h; U.log2W = log2W; U.log2H = log2H; U.m = m; U.maxVal = ( 1 << bd ) - 1;
    if( tid == 255 ) *s.dc = intraDcVal( U );
    __syncthreads();
    const int dcVal = *s.dc;

    for( int base = first; base < e; base += G )
    {
      const int job = base + g;
      bool      ok  = job < e;
      vtmhip_intra_job J;
      if( ok )
      {
        J  = jobs[job];
        ok = intraModeOk( J.mode, m );
      }
      int16_t *slot = FUSED ? s.pred + g * area : nullptr;
      if( ok )
      {
        vtmhip_intra_params p;
        intraPredParams( w, h, J.mode, m, p );
        IntraBlk b = U;
        if( p.refFilterFlag ) { b.top = sFTop; b.left = sFLeft; }
        int16_t *out = FUSED ? slot : predBase + J.predOff;
        if( RESI )
        {
          int16_t *res = resiBase + J.predOff;
          for( int i = l; i < area; i += L )
          {
            const int v = intraPredSample( p, J.mode, b, dcVal, c_intraCubic, i & ( w - 1 ), i >> log2W );
            out[i] = ( int16_t ) v;
            res[i] = ( int16_t ) ( s.org[i] - v );
          }
        }
        else
          for( int i = l; i < area; i += L ) out[i] = intraPredSample( p, J.mode, b, dcVal, c_intraCubic, i & ( w - 1 ), i >> log2W );
      }
      if( FUSED )
      {
        __syncthreads();
        if( L == 256 )
        {
          const int wv = tid >> 6;   // wave 0: SAD, wave 1: SATD
          if( ok && wv < 2 )
          {
            const unsigned long long d = wave_block_dist( wv ? VTMHIP_DIST_SATD : VTMHIP_DIST_SAD, s.org, w, slot, w, w, h, 0, tid & 63 );
            if( ( tid & 63 ) == 0 ) dist[2 * ( long ) job + wv] = d;
          }
        }
        else if( ok )
        {
          const unsigned long long sad  = lanes_block_dist<L>( VTMHIP_DIST_SAD, s.org, w, slot, w, w, h, 0, l );
          const unsigned long long satd = lanes_block_dist<L>( VTMHIP_DIST_SATD, s.org, w, slot, w, w, h, 0, l );
          if( l == 0 ) { dist[2 * ( long ) job] = sad; dist[2 * ( long ) job + 1] = satd; }
        }
        __syncthreads();   // before the next round overwrites the slots
      }
    }
  }
}

}   // namespace
