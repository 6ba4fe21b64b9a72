// intra_chroma_body.hpp -- the workgroup body of the intra chroma kernels, shared by intra_chroma.hip (intra_chroma_kernel: the two predictions alone, or kept in LDS
// and reduced to SAD and SATD) and intra_chroma_chain.hip (intra_chroma_resi_kernel: predictions and residuals).  How a workgroup walks its jobs is described in
// intra_chroma.hip.
#pragma once
#include "ctx.hpp"
#include "dist_block.hpp"
#include "cclm_rules.hpp"

namespace
{

constexpr int ICH_LINE     = 72;     // 2 * 32 + 1 samples of a line, rounded up
constexpr int ICH_MAX_AREA = 1024;
constexpr int ICH_EDGE     = 64;     // the top row / left column of the down-sampled luma: up to 2 * 32
constexpr int ICH_MIN_CHUNK = 8;

__host__ __device__ inline int ich_lanes( int maxArea ) { return maxArea <= 64 ? 16 : 64; }
__host__ __device__ inline int ich_chunk( int lanes ) { return lanes == 16 ? 16 : 8; }

__host__ __device__ inline CclmAvail ich_avail( const vtmhip_intra_chroma_block &b )
{
  const CclmAvail v = { b.above, b.left, b.aboveRight, b.belowLeft, b.firstRow, b.colocated };
  return v;
}
__host__ __device__ inline bool ich_block_ok( const vtmhip_intra_chroma_block &b ) { return cclmBlockOk( b.width, b.height, b.bitDepth, ich_avail( b ) ); }

// the staged down-sampled luma as cclmModel reads it
struct IchDs
{
  const int16_t *top, *left;
  __host__ __device__ int operator()( int i, int j ) const { return j < 0 ? top[i] : left[j]; }
};

struct IchLds
{
  int16_t   *line;    // [4][ICH_LINE]: Cb top, Cb left, Cr top, Cr left
  int16_t   *ds;      // [ICH_MAX_AREA] inner, [ICH_EDGE] top, [ICH_EDGE] left
  CclmModel *model;   // [3 modes][2 components]
  int       *dc;      // [2]
  int16_t   *org, *pred;   // org: fused and residual modes, [2][ICH_MAX_AREA]; pred: fused only, [G][2][area]
};

// what a job leaves behind: its two predictions in global memory; SAD and SATD of the predictions kept in LDS; predictions and residuals (original - prediction) in global memory
enum IchOut { ICH_OUT_PRED, ICH_OUT_DIST, ICH_OUT_RESI };

template<int L, IchOut OUT>
__device__ __forceinline__ void ich_chunk_body( const IchLds &s, const int16_t *__restrict__ refBase, const int16_t *__restrict__ lumaBase, const int16_t *__restrict__ orgBase,
                                                const vtmhip_intra_chroma_block *__restrict__ blocks, int numBlocks, const vtmhip_intra_chroma_job *__restrict__ jobs, int n,
                                                int16_t *__restrict__ predBase, unsigned long long *__restrict__ dist, int16_t *__restrict__ resiBase = nullptr )
{
  constexpr bool FUSED = OUT == ICH_OUT_DIST, RESI = OUT == ICH_OUT_RESI;
  constexpr int G = 256 / L, CHUNK = L == 16 ? 16 : 8;
  const int tid = threadIdx.x, g = tid / L, l = tid % L;
  const int jBegin = blockIdx.x * CHUNK, jEnd = min( n, jBegin + CHUNK );
  int16_t  *sDsTop = s.ds + ICH_MAX_AREA, *sDsLeft = sDsTop + ICH_EDGE;

  for( int j = jBegin; j < jEnd; )
  {
    // the run [j, e) of one block index (uniform over the workgroup)
    const int blk = uni( jobs[j].block );
    int       e   = j + 1;
    while( e < jEnd && uni( jobs[e].block ) == blk ) e++;
    const int first = j;
    j = e;
    if( blk < 0 || blk >= numBlocks ) continue;
    const vtmhip_intra_chroma_block B = blocks[blk];
    const int w = uni( ( int ) B.width ), h = uni( ( int ) B.height ), bd = uni( ( int ) B.bitDepth );
    CclmAvail V;
    V.above = uni( ( int ) B.above ); V.left = uni( ( int ) B.left ); V.aboveRight = uni( ( int ) B.aboveRight ); V.belowLeft = uni( ( int ) B.belowLeft );
    V.firstRow = uni( ( int ) B.firstRow ); V.colocated = uni( ( int ) B.colocated );
    if( !cclmBlockOk( w, h, bd, V ) || w * h > ( L == 16 ? 64 : ICH_MAX_AREA ) ) continue;   // the second part cannot happen: L comes from the largest block
    const int area = w * h, log2W = intraLog2( w ), log2H = intraLog2( h ), nTop = 2 * w + 1, nLeft = 2 * h + 1, maxVal = ( 1 << bd ) - 1;

    // does the run hold an LM job?  (a run has at most CHUNK <= 16 jobs)
    const int anyLm = __syncthreads_or( first + tid < e && cclmIsLm( jobs[first + tid].mode ) && cclmModeOk( jobs[first + tid].mode ) );   // also: the previous run's readers are done
    {
      const int nLine = nTop + nLeft;
      for( int i = tid; i < 2 * nLine; i += 256 )
      {
        const int c = i >= nLine, k = i - c * nLine;
        const int16_t v = refBase[( c ? B.crRefOff : B.cbRefOff ) + k];
        s.line[( 2 * c + ( k >= nTop ) ) * ICH_LINE + ( k >= nTop ? k - nTop : k )] = v;
      }
      if( FUSED || RESI )
        for( int i = tid; i < 2 * area; i += 256 )
        {
          const int c = i >= area, k = i - c * area;
          s.org[c * ICH_MAX_AREA + k] = orgBase[( c ? B.crOrgOff : B.cbOrgOff ) + ( long ) ( k >> log2W ) * B.orgStride + ( k & ( w - 1 ) )];
        }
      if( anyLm )
      {
        const CclmLuma luma = { lumaBase + B.lumaOff, B.lumaStride };
        const int reachT = cclmTopReach( w, h, V ), reachL = cclmLeftReach( w, h, V );
        for( int i = tid; i < area + reachT + reachL; i += 256 )
        {
          if( i < area ) s.ds[i] = ( int16_t ) cclmDsSample( luma, V, i & ( w - 1 ), i >> log2W );
          else if( i < area + reachT ) sDsTop[i - area] = ( int16_t ) cclmDsSample( luma, V, i - area, -1 );
          else sDsLeft[i - area - reachT] = ( int16_t ) cclmDsSample( luma, V, -1, i - area - reachT );
        }
      }
    }
    __syncthreads();
    IntraBlk U;   // of component c: the lines at ( 2 c, 2 c + 1 )
    U.w = w; U.h = h; U.log2W = log2W; U.log2H = log2H; U.m = 0; U.maxVal = maxVal;
    if( tid >= 254 || ( anyLm && tid < 6 ) )
    {
      const int c = tid & 1;
      U.top = s.line + 2 * c * ICH_LINE; U.left = U.top + ICH_LINE;
      if( tid >= 254 ) s.dc[c] = intraDcVal( U );
      else
      {
        const IchDs ds = { sDsTop, sDsLeft };
        s.model[tid] = cclmModel( w, h, CCLM_LM + ( tid >> 1 ), bd, V, U.top, U.left, ds );
      }
    }
    __syncthreads();

    for( int base = first; base < e; base += G )
    {
      const int job = base + g;
      bool      ok  = job < e;
      vtmhip_intra_chroma_job J;
      if( ok )
      {
        J  = jobs[job];
        ok = cclmModeOk( J.mode );
      }
      int16_t *slot = FUSED ? s.pred + g * 2 * area : nullptr;
      if( ok )
      {
        if( cclmIsLm( J.mode ) )
        {
          for( int i = l; i < 2 * area; i += L )
          {
            const int c = i >= area, k = i - c * area;
            const int16_t v = cclmPredSample( s.model[2 * ( J.mode - CCLM_LM ) + c], s.ds[k], maxVal );
            if( FUSED ) slot[i] = v;
            else predBase[( c ? J.crPredOff : J.cbPredOff ) + k] = v;
            if( RESI ) resiBase[( c ? J.crPredOff : J.cbPredOff ) + k] = ( int16_t ) ( s.org[c * ICH_MAX_AREA + k] - v );
          }
        }
        else
        {
          vtmhip_intra_params p;
          intraPredParams( w, h, J.mode, 0, p, true );
          for( int i = l; i < 2 * area; i += L )
          {
            const int c = i >= area, k = i - c * area;
            U.top = s.line + 2 * c * ICH_LINE; U.left = U.top + ICH_LINE;
            const int16_t v = intraPredSample( p, J.mode, U, s.dc[c], nullptr, k & ( w - 1 ), k >> log2W, true );
            if( FUSED ) slot[i] = v;
            else predBase[( c ? J.crPredOff : J.cbPredOff ) + k] = v;
            if( RESI ) resiBase[( c ? J.crPredOff : J.cbPredOff ) + k] = ( int16_t ) ( s.org[c * ICH_MAX_AREA + k] - v );
          }
        }
      }
      if( FUSED )
      {
        __syncthreads();
        if( ok )
        {
#pragma unroll 1
          for( int c = 0; c < 2; c++ )   // one copy of the two reductions
          {
            const unsigned long long sad  = lanes_block_dist<L>( VTMHIP_DIST_SAD, s.org + c * ICH_MAX_AREA, w, slot + c * area, w, w, h, 0, l );
            const unsigned long long satd = lanes_block_dist<L>( VTMHIP_DIST_SATD, s.org + c * ICH_MAX_AREA, w, slot + c * area, w, w, h, 0, l );
            if( l == 0 ) { dist[4 * ( long ) job + 2 * c] = sad; dist[4 * ( long ) job + 2 * c + 1] = satd; }
          }
        }
        __syncthreads();   // before the next round overwrites the slots
      }
    }
  }
}

}   // namespace
