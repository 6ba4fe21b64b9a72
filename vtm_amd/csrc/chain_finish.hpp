// chain_finish.hpp -- the last step of a level entry's residual chain, shared by intra_chain_finish_kernel (intra_chain.hip) and intra_chroma_chain_finish_kernel
// (intra_chroma_chain.hip): the reconstructed residual becomes the clipped reconstruction, and its SSE against the original joins what the chain left.
// An item (one component block) gets L lanes: 16 up to 256 samples, sixteen items per workgroup; 64 above, a wave per item.  The kernels decode their own items
// and call
//   chain_finish_walk<L>       a lane walks 4-sample row segments: prediction and reconstructed residual are W x H contiguous, the original has its own stride; all
//                              three come as one 8-byte access at a 2-byte aligned address (pel_pack.hpp).  It overwrites the reconstructed residual with
//                              clip( prediction + residual ) and sums ( original - reconstruction )^2 with the per-addend 32-bit product of dist_block.hpp's SSE
//   chain_finish_group_sum<L>  the item's lanes added by shuffles.  No LDS, no barrier
//   chain_finish_result        the chain's vtmhip_tu_result and the SSE as a vtmhip_intra_tu_result
// and the entries launch them through chain_finish_launch, which picks L from the largest item.
#pragma once
#include "ctx.hpp"
#include "intra_rules.hpp"   // intraLog2
#include "pel_pack.hpp"

template<int L>
__device__ __forceinline__ unsigned long long chain_finish_walk( const int16_t *pred, int16_t *reco, const int16_t *org, int orgStride, int width, int height, int bitDepth, int l )
{
  const int lgSegs = intraLog2( width ) - 2, items = ( width * height ) >> 2, maxVal = ( 1 << bitDepth ) - 1;
  unsigned long long acc = 0;
  for( int it = l; it < items; it += L )
  {
    const int y = it >> lgSegs, x = ( it & ( ( 1 << lgSegs ) - 1 ) ) << 2;
    int p[4], r[4], o[4];
    ld4( pred + 4 * it, 4, p );
    ld4( reco + 4 * it, 4, r );
    ld4( org + ( long ) y * orgStride + x, 4, o );
#pragma unroll
    for( int k = 0; k < 4; k++ )
    {
      r[k] = min( max( p[k] + r[k], 0 ), maxVal );
      const int d = o[k] - r[k];
      acc += ( unsigned long long ) ( ( unsigned ) d * ( unsigned ) d );
    }
    st4( reco + 4 * it, 4, r );
  }
  return acc;
}

// a group is L consecutive lanes of one wave; every lane of the wave calls this
template<int L>
__device__ __forceinline__ unsigned long long chain_finish_group_sum( unsigned long long acc )
{
#pragma unroll
  for( int o = L >> 1; o > 0; o >>= 1 ) acc += __shfl_xor( acc, o, 64 );
  return acc;
}

__device__ __forceinline__ vtmhip_intra_tu_result chain_finish_result( unsigned long long sse, const vtmhip_tu_result &t )
{
  vtmhip_intra_tu_result r;
  r.sse = sse; r.sseResi = t.sse; r.sumAbs = t.sumAbs; r.absSum = t.absSum;
  return r;
}

// k16 / k64: the two instantiations of a finish kernel; 256 threads, `items` items, the largest of them maxArea samples
template<class... P, class... A>
int chain_finish_launch( vtmhip_ctx *ctx, const char *name, void ( *k16 )( P... ), void ( *k64 )( P... ), int maxArea, int items, A... args )
{
  const bool narrow = maxArea <= 256;
  const int  perGroup = narrow ? 16 : 4;
  void ( *const kernel )( P... ) = narrow ? k16 : k64;
  VTMHIP_TIME_KERNEL( ctx, name );
  hipLaunchKernelGGL( kernel, dim3( ( items + perGroup - 1 ) / perGroup ), dim3( 256 ), 0, ctx->stream, args... );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}
