// mc_sinks.hpp -- output sinks of mc_block / mc_block_vec (mc_block.hpp) that keep a prediction in LDS, shared by the kernels that predict a block and consume it
// where it lies: mmvd.hip (the MMVD candidates) and ciip.hip (the CIIP candidates).
#pragma once
#include "mc_block.hpp"

namespace
{

enum { AVG_BCW_DEFAULT = 4 };   // the list-1 weight of 8 that means addAvg

struct ToLds
{
  int16_t *p; int w;
  __device__ __forceinline__ void operator()( int y, int x, int16_t v ) const { p[y * w + x] = v; }
  __device__ __forceinline__ void vec( int y, int x0, const int v[8] ) const { *reinterpret_cast<uint4 *>( p + y * w + x0 ) = pack8( v ); }
};
// the list-1 block meets the list-0 block where it lies: addAvg (Buffer.cpp:467-507) or, under a BCW weight, addWeightedAvg (Buffer.cpp:365-397; bcw = the list-1
// weight of 8) written over it.  Every sample is read and written by one lane.
struct AvgOver
{
  int16_t *p; int w; int shift, cmax, bcw;
  __device__ __forceinline__ int one( int a, int b ) const
  {
    const int v = bcw == AVG_BCW_DEFAULT ? ( a + b + ( 1 << ( shift - 1 ) ) + 2 * 8192 ) >> shift : ( a * ( 8 - bcw ) + b * bcw + ( 1 << ( shift + 1 ) ) + ( 8192 << 3 ) ) >> ( shift + 2 );
    return min( cmax, max( 0, v ) );
  }
  __device__ __forceinline__ void operator()( int y, int x, int16_t v ) const { p[y * w + x] = ( int16_t ) one( p[y * w + x], v ); }
  __device__ __forceinline__ void vec( int y, int x0, const int v[8] ) const
  {
    int a[8], r[8];
    load8s( p + y * w + x0, a );
#pragma unroll
    for( int k = 0; k < 8; k++ ) r[k] = one( a[k], v[k] );
    *reinterpret_cast<uint4 *>( p + y * w + x0 ) = pack8( r );
  }
};

}   // namespace
