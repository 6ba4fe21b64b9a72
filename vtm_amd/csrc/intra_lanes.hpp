// intra_lanes.hpp -- how the intra kernels that work from a vtmhip_intra_block table (intra.hip: the regular modes, mip.hip: MIP) divide a workgroup among jobs, defined
// once: a job gets 16, 64 or 256 lanes by the largest well-formed block of the table, a workgroup takes 16 / 8 / 4 consecutive jobs, and intra_shape_kernel -- one
// workgroup -- leaves the lane count in device memory so that the host never waits for the table.
#pragma once
#include "ctx.hpp"
#include "intra_rules.hpp"
#include "intra_lane_rule.hpp"   // intra_lanes, intra_chunk, INTRA_MAX_AREA, INTRA_MIN_CHUNK: the rule without the kernel

namespace
{

__device__ __forceinline__ bool intra_block_ok( const vtmhip_intra_block &b ) { return intraBlockOk( b.width, b.height, b.bitDepth, b.multiRefIdx ); }

__global__ __launch_bounds__( 256 ) void intra_shape_kernel( const vtmhip_intra_block *__restrict__ blocks, int numBlocks, int *__restrict__ lanes )
{
  __shared__ int sMax;
  if( threadIdx.x == 0 ) sMax = 16;
  __syncthreads();
  int m = 0;
  for( int i = threadIdx.x; i < numBlocks; i += 256 )
  {
    const vtmhip_intra_block b = blocks[i];
    if( intra_block_ok( b ) ) m = max( m, b.width * b.height );
  }
  if( m ) atomicMax( &sMax, m );
  __syncthreads();
  if( threadIdx.x == 0 ) *lanes = intra_lanes( sMax );
}

}   // namespace
