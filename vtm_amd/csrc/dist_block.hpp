// dist_block.hpp -- the distortion of ONE (original block, candidate block) pair: SAD with row sub-sampling (RdCost.cpp:493-1003), SSE (:1783-2133) or SATD by the tile
// rule of xGetHADs (had_tile_shape, had.hpp).  block_dist_walk is the walk over the block's work items -- 4-sample row segments (single samples for widths like 2 / 6),
// Hadamard tiles -- by one lane of a group of any size: items first, first + step, ...; it returns that lane's partial sum and the caller reduces it its own way.
// lanes_block_dist<L> is the walk by a group of L <= 64 consecutive lanes of a wave (L a power of two, `lane` the index inside the group) plus the shuffle reduction: the
// result is in every lane of the group, so small blocks share a wave, one block per group; wave_block_dist is the L = 64 case.  Callers: dist.hip, mest.hip, the intra /
// MIP / chroma bodies (the shuffle forms); interp.hip, smvd.hip, affine.hip, mmvd.hip (the walk, with a workgroup's reduction).
#pragma once
#include "ctx.hpp"
#include "had.hpp"

__device__ __forceinline__ unsigned long long block_dist_walk( int kind, const int16_t *org, int os, const int16_t *cur, int cs, int w, int h, int subShift, int first, int step )
{
  unsigned long long acc = 0;

  if( kind == VTMHIP_DIST_SAD )
  {
    // rows y = 0, 1 << ss, 2 << ss ...; work items = (row, 4-sample segment), or single samples for widths like 2 / 6 (chroma)
    const int ss = subShift, rows = ( h + ( 1 << ss ) - 1 ) >> ss, segs = w >> 2;
    unsigned  s = 0;
    if( ( w & 3 ) == 0 )
    {
      for( int it = first; it < rows * segs; it += step )
      {
        const int      r = it / segs, x = ( it - r * segs ) << 2;
        const int16_t *o = org + ( long ) ( r << ss ) * os + x;
        const int16_t *c = cur + ( long ) ( r << ss ) * cs + x;
#pragma unroll
        for( int k = 0; k < 4; k++ ) s += ( unsigned ) abs( ( int ) o[k] - ( int ) c[k] );
      }
    }
    else
    {
      for( int it = first; it < rows * w; it += step )
      {
        const int r = it / w, x = it - r * w;
        s += ( unsigned ) abs( ( int ) org[( long ) ( r << ss ) * os + x] - ( int ) cur[( long ) ( r << ss ) * cs + x] );
      }
    }
    acc = ( unsigned long long ) s << ss;   // per-lane partial (W*H*65535 < 2^32 for W,H <= 128 needs care: 128*128*65535 = 2^30)
  }
  else if( kind == VTMHIP_DIST_SSE )
  {
    const int segs = w >> 2;
    if( ( w & 3 ) == 0 )
    {
      for( int it = first; it < h * segs; it += step )
      {
        const int      r = it / segs, x = ( it - r * segs ) << 2;
        const int16_t *o = org + ( long ) r * os + x;
        const int16_t *c = cur + ( long ) r * cs + x;
#pragma unroll
        for( int k = 0; k < 4; k++ )
        {
          const int d = ( int ) o[k] - ( int ) c[k];
          acc += ( unsigned long long ) ( ( unsigned ) d * ( unsigned ) d );   // per-addend 32-bit product as RdCost.cpp:1783-1814
        }
      }
    }
    else
    {
      for( int it = first; it < h * w; it += step )
      {
        const int r = it / w, x = it - r * w;
        const int d = ( int ) org[( long ) r * os + x] - ( int ) cur[( long ) r * cs + x];
        acc += ( unsigned long long ) ( ( unsigned ) d * ( unsigned ) d );
      }
    }
  }
  else   // SATD: one tile per item
  {
    const HadTile t = had_tile_shape( w, h );
    const int     tx = w / t.w, ty = h / t.h;
    for( int it = first; it < tx * ty; it += step )
    {
      const int y = ( it / tx ) * t.h, x = ( it % tx ) * t.w;
      acc += had_tile_of( t, org + ( long ) y * os + x, os, cur + ( long ) y * cs + x, cs );
    }
  }
  return acc;
}

template<int L>
__device__ __forceinline__ unsigned long long lanes_block_dist( int kind, const int16_t *org, int os, const int16_t *cur, int cs, int w, int h, int subShift, int lane )
{
  unsigned long long acc = block_dist_walk( kind, org, os, cur, cs, w, h, subShift, lane, L );
#pragma unroll
  for( int o = L >> 1; o > 0; o >>= 1 ) acc += __shfl_xor( acc, o, 64 );
  return acc;
}

__device__ __forceinline__ unsigned long long wave_block_dist( int kind, const int16_t *org, int os, const int16_t *cur, int cs, int w, int h, int subShift, int lane )
{
  return lanes_block_dist<64>( kind, org, os, cur, cs, w, h, subShift, lane );
}
