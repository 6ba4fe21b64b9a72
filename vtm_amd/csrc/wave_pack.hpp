// wave_pack.hpp -- several small jobs per wave, the skeleton of the per-block batch kernels (sse_wtd_kernel, wp_dist_kernel, lmcs_op_kernel): a wave takes a GROUP
// of G consecutive jobs (G <= 64, chosen by the host from n); lane i < G validates job i of the group, builds its LDS record and counts its ITEMS (4-sample row
// segments, rows, Hadamard tiles; 0 rejects the job); a wave prefix scan of the counts lays the items of all G jobs end to end, and the lanes walk them -- lane-
// strided or in wave-uniform steps of 64 -- with a cursor that finds the job of an item: 2x2 / 4x4 blocks share a wave, a 128x128 block keeps all lanes busy.
// The part without HIP (launch rules, group indexing, FastDiv, the cursor) runs in host/test_wave_pack.cpp under sanitizers.
#pragma once
#include <cstdint>

#if defined( __HIPCC__ )
#define WAVE_PACK_HD __host__ __device__ __forceinline__
#else
#define WAVE_PACK_HD inline
#endif

// jobs per wave: pack as many as still leave ~32 waves per CU (8 per SIMD, what the latency of the sample loads needs), at most 64
WAVE_PACK_HD int wave_jobs_per_wave( int numCUs, int n )
{
  const int g = n / ( numCUs * 32 );
  return g < 1 ? 1 : g > 64 ? 64 : g;
}
WAVE_PACK_HD int wave_groups( int n, int G ) { return ( n + G - 1 ) / G; }
// workgroups of `waves` waves, a group per wave, at most maxBlocks of them: the kernels loop over the rest
WAVE_PACK_HD int wave_blocks( int n, int G, int waves, int maxBlocks )
{
  const int blocks = ( wave_groups( n, G ) + waves - 1 ) / waves;
  return blocks > maxBlocks ? maxBlocks : blocks;
}

// p / d for 0 <= p with p * d < 2^32: multiply-high by floor((2^32 - 1) / d) and one correction step (4 instructions) instead of the generic ~25-instruction
// integer division sequence; the constructor's division is once per block / per job
struct FastDiv
{
  int d; unsigned magic;
  FastDiv() = default;
  WAVE_PACK_HD explicit FastDiv( int dd ) : d( dd ), magic( 0xffffffffu / ( unsigned ) dd ) {}
  WAVE_PACK_HD int operator()( int p ) const
  {
#if defined( __HIP_DEVICE_COMPILE__ )
    const int q = ( int ) __umulhi( ( unsigned ) p, magic );
#else
    const int q = ( int ) ( ( ( uint64_t ) ( unsigned ) p * magic ) >> 32 );
#endif
    return q + ( ( q + 1 ) * d <= p ? 1 : 0 );
  }
};

// the job of a lane's current item: items [start, end) belong to job cj of the group.  A lane's items only grow, so the cursor only moves forward.
struct WaveCursor
{
  int cj = -1, start = 0, end = 0;
  WAVE_PACK_HD bool beyond( int t ) const { return t >= end; }
  // ends[]: the inclusive prefix of the group's item counts; t < ends[last].  Skips jobs without items (rejected ones).
  WAVE_PACK_HD void advance( int t, const int *ends ) { do { start = end; end = ends[++cj]; } while( t >= end ); }
};

// wave `wv` of a workgroup whose first group is `round`: its group, the group's first job, the lane's job, and whether that job exists
struct WaveGroup
{
  int grp, base, job; bool mine;
  WAVE_PACK_HD WaveGroup( int round, int wv, int lane, int n, int G, int nGroups )
    : grp( round + wv ), base( grp * G ), job( base + lane ), mine( grp < nGroups && lane < G && job < n ) {}
};

#if defined( __HIPCC__ )
// inclusive prefix of the 64 lanes' item counts into ends[lane]; returns the group's total
__device__ __forceinline__ int wave_scan_items( int lane, int items, int *ends )
{
  int incl = items;
#pragma unroll
  for( int o = 1; o < 64; o <<= 1 )
  {
    const int t = __shfl_up( incl, o, 64 );
    if( lane >= o ) incl += t;
  }
  const int total = __shfl( incl, 63, 64 );
  ends[lane] = incl;
  return total;
}
#endif
