// mip_body.hpp -- the workgroup body of the MIP kernels, shared by mip.hip (mip_kernel: the prediction alone, or kept in LDS and reduced to SAD and SATD) and
// intra_chain.hip (mip_resi_kernel: prediction and residual).  How a workgroup walks its jobs is described in mip.hip.
#pragma once
#include "ctx.hpp"
#include "dist_block.hpp"
#include "intra_lane_rule.hpp"
#include "mip_rules.hpp"

namespace
{

constexpr int MIP_LINE      = 72;   // indices 1 .. 64 of a line, rounded up
constexpr int MIP_TAB_BYTES = MIP_BYTES_4X4 + MIP_BYTES_8X8 + MIP_BYTES_16X16;

struct MipLds
{
  int16_t *line;   // [2][MIP_LINE]: top, left, indexed as the block's lines are (1 .. W, 1 .. H)
  int     *bdry;   // [2][4]: reduced top, reduced left
  int     *in;     // [2][MIP_MAX_INPUT]: the rebased input, top | left then left | top
  int16_t *red;    // [16][MIP_MAX_REDUCED]: a reduced block per lane group
  int16_t *org, *pred;   // org: fused and residual modes; pred: fused only
};

enum MipOut { MIP_OUT_PRED, MIP_OUT_DIST, MIP_OUT_RESI };   // as IntraOut (intra_body.hpp)

template<int L, MipOut OUT>
__device__ __forceinline__ void mip_chunk_body( const MipLds &s, const uint8_t *__restrict__ tab, const int16_t *__restrict__ refBase, const int16_t *__restrict__ orgBase,
                                                const vtmhip_intra_block *__restrict__ blocks, int numBlocks, const vtmhip_mip_job *__restrict__ jobs, int n,
                                                int16_t *__restrict__ predBase, unsigned long long *__restrict__ dist, int16_t *__restrict__ resiBase = nullptr )
{
  constexpr bool FUSED = OUT == MIP_OUT_DIST, RESI = OUT == MIP_OUT_RESI;
  constexpr int G = 256 / L, CHUNK = L == 16 ? 16 : L == 64 ? 8 : 4;
  const int tid = threadIdx.x, g = tid / L, l = tid % L;
  const int jBegin = blockIdx.x * CHUNK, jEnd = min( n, jBegin + CHUNK );
  int16_t  *sTop = s.line, *sLeft = s.line + MIP_LINE;

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
    if( !mipBlockOk( w, h, bd, m ) || w * h > ( L == 16 ? 64 : L == 64 ? 1024 : INTRA_MAX_AREA ) ) continue;   // the second part cannot happen: L comes from the largest block
    const MipShape S = mipShape( w, h );
    const int area = w * h, log2W = mipLog2( w ), nRed = S.pred * S.pred;

    __syncthreads();   // the previous run's readers are done
    {
      const int16_t *ref = refBase + B.refOff;   // top[i] = ref[i], left[i] = ref[2W + 1 + i]
      for( int i = tid; i < w + h; i += 256 )
      {
        if( i < w ) sTop[1 + i] = ref[1 + i];
        else sLeft[1 + i - w] = ref[2 * w + 2 + i - w];
      }
      if( FUSED || RESI )
      {
        const int16_t *org = orgBase + B.orgOff;
        for( int i = tid; i < area; i += 256 ) s.org[i] = org[( long ) ( i >> log2W ) * B.orgStride + ( i & ( w - 1 ) )];
      }
    }
    __syncthreads();
    if( tid < 2 * S.bdry )
    {
      const int t = tid >= S.bdry, i = tid - t * S.bdry;
      s.bdry[4 * t + i] = mipBoundarySample( t ? sLeft : sTop, t ? h : w, S.bdry, i );
    }
    __syncthreads();
    if( tid < 2 * MIP_MAX_INPUT && ( tid & 7 ) < 2 * S.bdry )
    {
      const int t = tid >> 3;   // 0: top | left, 1: left | top
      s.in[tid] = mipInputAt( S, bd, s.bdry + 4 * t, s.bdry + 4 * ( 1 - t ), tid & 7 );
    }
    __syncthreads();

    for( int base = first; base < e; base += G )
    {
      const int job = base + g;
      bool      ok  = job < e;
      vtmhip_mip_job J;
      if( ok )
      {
        J  = jobs[job];
        ok = mipJobOk( S, J.mode, J.transposed );
      }
      int16_t *red = s.red + g * MIP_MAX_REDUCED, *slot = FUSED ? s.pred + g * area : nullptr;
      if( ok )
      {
        const int      t      = J.transposed;
        const uint8_t *matrix = mipMatrix( S, J.mode, tab, tab + MIP_BYTES_4X4, tab + MIP_BYTES_4X4 + MIP_BYTES_8X8 );
        for( int pos = l; pos < nRed; pos += L ) red[mipRedIndex( S, t, pos )] = ( int16_t ) mipReducedSample( S, s.in + MIP_MAX_INPUT * t, s.bdry[4 * t], bd, matrix, pos );
      }
      __syncthreads();
      if( ok )
      {
        int16_t *out = FUSED ? slot : predBase + J.predOff;
        if( RESI )
        {
          int16_t *res = resiBase + J.predOff;
          for( int i = l; i < area; i += L )
          {
            const int v = mipSample( S, red, sTop, sLeft, i & ( w - 1 ), i >> log2W );
            out[i] = ( int16_t ) v;
            res[i] = ( int16_t ) ( s.org[i] - v );
          }
        }
        else
          for( int i = l; i < area; i += L ) out[i] = mipSample( S, red, sTop, sLeft, i & ( w - 1 ), i >> log2W );
      }
      __syncthreads();   // the reduced blocks are free again; fused: the slots are complete
      if( FUSED )
      {
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
