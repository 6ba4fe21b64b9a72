// geo.hip -- the GEO candidates of the merge pre-selection (EncCu::xCheckRDCostMergeGeo2Nx2N, EncCu.cpp:2811-3031; hook B10) and the RD stage's blend (:3023-3031, :3073).
//   vtmhip_geo_cand_satd_batch_dev   per CU: the candidates' 14-bit uni-predictions -> optional kept stores -> whole-block and 64 x numCand masked SADs of the rounded
//                                    blocks -> cost filter -> ordered list -> per listed combination blend + SATD / SAD: the result record, the optional sadLarge
//                                    table and the kept blocks are all that is stored
//   vtmhip_geo_blend_batch_dev       weightedGeoBlk for luma and 4:2:0 chroma blocks, the weights from the closed form
//   vtmhip_geo_host / vtmhip_geo_tables_host   the same as host arithmetic (geo_host.hpp)
// The rules are geo_rules.hpp's: no weight or mask plane exists on the device.  The motion compensation is mc_any (mc_block.hpp) with bi = 1 and the ToLds sink of
// mc_sinks.hpp, the distortion block_dist_walk (dist_block.hpp).
//
// geo_fused_kernel<THREADS>: one workgroup of THREADS lanes per CU, THREADS = vtmhip_geo_lanes_per_job( maxWidth, maxHeight ): 64 up to 1024 samples, 256 above.
// The workgroup checks its job (geoJobOk; a malformed job leaves the skipped record and nothing else), loads the original block into LDS, and lanes 0 .. 63 each form
// the weight-index line (c0, cx, cy) of one split.  Then
//   - per candidate mc_any into its own LDS block (14 bit), and the kept stores;
//   - per candidate | org - round( pred ) | once per sample into the scratch block, its sum (the whole-block SAD), and the 64 masked SADs: lane & 63 is the split,
//     every lane of a wave reads the same 8 differences (an LDS broadcast) and adds those whose weight index is positive; with 256 lanes the four waves take
//     every fourth segment and meet in an LDS atomic.  No cross-lane reduction is needed;
//   - the filter: every lane walks its share of the 64 x numCand x ( numCand - 1 ) combinations and appends the kept ones (cost bits, splitDir * 32 + pair) through
//     an LDS counter; the order of arrival does not matter because the list order is total;
//   - a bitonic sort of the list, padded to a power of two, in LDS;
//   - per listed combination, up to 60: the blend of the two 14-bit blocks into the scratch block and block_dist_walk from LDS.
// LDS per workgroup: original + six candidates (7 x maxW x maxH x 2 B), the scratch block (maxW x ( maxH + 7 ) x 2 B: the H-pass intermediates, the differences,
// the blended block), the list (2048 x ( 8 + 2 ) B = 20 KB), sadLarge, the whole SADs, the lines and the counter (2.3 KB):
//   <64>    8 x 8     23.4 KB   <64>   16 x 16   26.5 KB   <64>   32 x 32 / 64 x 16   38.7 KB   <256>  64 x 64   87.2 KB
// Workgroups per compute unit by division into its 160 KB (arithmetic, not a measurement; the allocation is rounded up to a granule this file does not know, which at
// 16 x 16 -- 6.03 by the plain quotient -- decides between 5 and 6): 6, 5 or 6, 4 and 1, that is 1.5, 1.25 - 1.5, 1 and 1 waves per SIMD.
// (at 64 x 64 the seven blocks and the scratch alone are 64.9 KB).  Registers and scratch of both instantiations: profiles/geo_kernel_resources.txt.
//
// geo_blend_kernel: 256 threads, 64 lanes per job, four jobs per workgroup; a sample per lane and step.
#include <atomic>

#include "ctx.hpp"
#include "mc_block.hpp"
#include "mc_sinks.hpp"
#include "dist_block.hpp"
#include "geo_rules.hpp"
#include "geo_host.hpp"   // the host entries' bodies: shared with host/test_geo_cand.cpp

namespace
{

constexpr unsigned long long GEO_NO_COST = ~0ull;
constexpr int                GEO_LIST_CAP = 2048;   // the power of two above GEO_MAX_COMBOS = 1920
constexpr int                GEO_MAX_DEVICES = 64;

__host__ __device__ inline int geo_scratch_samples( int maxW, int maxH ) { return ( maxW * ( maxH + 7 ) + 7 ) & ~7; }
__host__ __device__ inline size_t geo_lds_bytes( int maxW, int maxH )
{
  return ( size_t ) ( 7 * maxW * maxH + geo_scratch_samples( maxW, maxH ) ) * sizeof( int16_t ) + GEO_LIST_CAP * ( sizeof( unsigned long long ) + sizeof( unsigned short ) ) +
         ( GEO_NUM_SPLIT * VTMHIP_GEO_MAX_CAND + 8 + 3 * GEO_NUM_SPLIT + 4 ) * sizeof( int );
}

// a result slot as three 64-bit words: cost, dist, splitDir | cand0 << 8 | cand1 << 16 (the pad bytes are zero)
__device__ __forceinline__ void geo_store_combo( vtmhip_geo_combo *c, unsigned long long costBits, unsigned long long dist, unsigned split, unsigned cand0, unsigned cand1 )
{
  unsigned long long *p = reinterpret_cast<unsigned long long *>( c );
  p[0] = costBits; p[1] = dist; p[2] = split | ( cand0 << 8 ) | ( cand1 << 16 );
}

template<int THREADS>
__global__ __launch_bounds__( THREADS ) void geo_fused_kernel( const int16_t *__restrict__ refBase, const int16_t *__restrict__ orgBase, int16_t *predBase,
                                                               const vtmhip_geo_job *__restrict__ jobs, int n, int maxW, int maxH, int useSatd,
                                                               vtmhip_geo_result *__restrict__ results, unsigned long long *__restrict__ sadSplit )
{
  extern __shared__ __attribute__( ( aligned( 16 ) ) ) int16_t lds[];
  __shared__ unsigned long long sCost;   // THREADS == 256: the block's cost
  constexpr int NP = THREADS / 64;       // waves of the workgroup
  const int lane = ( int ) threadIdx.x;
  const int item = xcd_order( ( int ) blockIdx.x, ( int ) gridDim.x );
  if( item >= n ) return;
  const vtmhip_geo_job &j   = jobs[item];
  vtmhip_geo_result    &out = results[item];
  unsigned long long   *splitOut = sadSplit ? sadSplit + ( long ) GEO_NUM_SPLIT * VTMHIP_GEO_MAX_CAND * item : nullptr;
  if( !geoJobOk( j, maxW, maxH, predBase != nullptr ) )   // uniform over the workgroup
  {
    if( lane < VTMHIP_GEO_MAX_CAND ) out.sadWhole[lane] = GEO_NO_COST;
    if( lane == 0 ) { out.numPassed = 0; out.numTested = 0; }
    for( int r = lane; r < VTMHIP_GEO_MAX_TRY; r += THREADS ) geo_store_combo( &out.combo[r], 0, GEO_NO_COST, 0, 0, 0 );
    if( splitOut )
      for( int i = lane; i < GEO_NUM_SPLIT * VTMHIP_GEO_MAX_CAND; i += THREADS ) splitOut[i] = GEO_NO_COST;
    return;
  }
  const int    w = j.width, h = j.height, bd = j.bitDepth, lgW = 31 - __clz( w ), area = w * h, segs = area >> 3, numCand = j.numCand, A = maxW * maxH;
  const double lambda = j.sqrtLambda;
  int16_t *orgL = lds, *pred = orgL + A, *tmp = pred + VTMHIP_GEO_MAX_CAND * A;
  unsigned long long *key  = reinterpret_cast<unsigned long long *>( tmp + geo_scratch_samples( maxW, maxH ) );
  unsigned           *sadL = reinterpret_cast<unsigned *>( key + GEO_LIST_CAP ), *sadW = sadL + GEO_NUM_SPLIT * VTMHIP_GEO_MAX_CAND;
  int                *line = reinterpret_cast<int *>( sadW + 8 ), *cnt = line + 3 * GEO_NUM_SPLIT;
  unsigned short     *idx  = reinterpret_cast<unsigned short *>( cnt + 4 );

  {
    const int16_t *org = orgBase + j.orgOff;
    for( int i = lane; i < area; i += THREADS ) orgL[i] = org[( long ) ( i >> lgW ) * j.orgStride + ( i & ( w - 1 ) )];
    for( int i = lane; i < GEO_NUM_SPLIT * VTMHIP_GEO_MAX_CAND + 8; i += THREADS ) sadL[i] = 0;   // sadLarge and the whole SADs
    if( lane < GEO_NUM_SPLIT )
    {
      const GeoLine l = geoLine( lane, w, h, 0, 0 );
      line[3 * lane] = l.c0; line[3 * lane + 1] = l.cx; line[3 * lane + 2] = l.cy;
    }
    if( lane == 0 ) cnt[0] = 0;
  }
  // ---- the candidates as 14-bit intermediates ----
  for( int c = 0; c < numCand; c++ )
  {
    const vtmhip_geo_cand &cd = j.cand[c];
    vtmhip_mc_job          m;
    m.width = ( int16_t ) w; m.height = ( int16_t ) h; m.bitDepth = ( uint8_t ) bd; m.useAltHpelIf = 0; m.chroma = 0; m.bi = 1; m.dstOff = 0; m.dstStride = 0;
    m.refOff = cd.refOff; m.refStride = cd.refStride; m.mvHor = cd.mv[0]; m.mvVer = cd.mv[1];
    block_sync<THREADS>();   // the previous candidate's H-pass intermediates have been read
    mc_any<THREADS>( m, refBase, tmp, lane, ToLds{ pred + c * A, w } );
  }
  block_sync<THREADS>();
  for( int c = 0; c < numCand; c++ )
  {
    if( j.cand[c].keepOff < 0 ) continue;
    int16_t *keep = predBase + j.cand[c].keepOff;
    for( int s = lane; s < segs; s += THREADS )
    {
      int v[8];
      load8s( pred + c * A + 8 * s, v );
      store8g( keep + 8 * s, v );
    }
  }
  // ---- whole-block and masked SADs of the rounded blocks ----
  for( int c = 0; c < numCand; c++ )
  {
    block_sync<THREADS>();   // the scratch block's readers are done
    unsigned whole = 0;
    for( int s = lane; s < segs; s += THREADS )
    {
      int v[8], o[8];
      load8s( pred + c * A + 8 * s, v );
      load8s( orgL + 8 * s, o );
#pragma unroll
      for( int t = 0; t < 8; t++ ) { v[t] = abs( o[t] - geoRoundSample( v[t], bd ) ); whole += ( unsigned ) v[t]; }
      *reinterpret_cast<uint4 *>( tmp + 8 * s ) = pack8( v );
    }
    whole = ( unsigned ) wave_reduce_add( ( int ) whole );
    if( ( lane & 63 ) == 0 ) atomicAdd( &sadW[c], whole );
    block_sync<THREADS>();
    const int split = lane & 63, c0 = line[3 * split], cx = line[3 * split + 1], cy = line[3 * split + 2];
    unsigned  acc = 0;
    for( int s = lane >> 6; s < segs; s += NP )
    {
      int d[8];
      load8s( tmp + 8 * s, d );   // one address per wave: a broadcast
      const int base = c0 + cx * ( ( 8 * s ) & ( w - 1 ) ) + cy * ( ( 8 * s ) >> lgW );
#pragma unroll
      for( int t = 0; t < 8; t++ ) acc += geoMaskOfIdx( base + cx * t ) ? ( unsigned ) d[t] : 0u;
    }
    if( NP == 1 ) sadL[split * VTMHIP_GEO_MAX_CAND + c] = acc;
    else atomicAdd( &sadL[split * VTMHIP_GEO_MAX_CAND + c], acc );
  }
  block_sync<THREADS>();
  uint64_t whole[VTMHIP_GEO_MAX_CAND];
#pragma unroll
  for( int c = 0; c < VTMHIP_GEO_MAX_CAND; c++ ) whole[c] = c < numCand ? ( uint64_t ) sadW[c] : GEO_NO_COST;
  if( lane < VTMHIP_GEO_MAX_CAND ) out.sadWhole[lane] = lane < numCand ? ( unsigned long long ) sadW[lane] : GEO_NO_COST;
  if( splitOut )
    for( int i = lane; i < GEO_NUM_SPLIT * VTMHIP_GEO_MAX_CAND; i += THREADS ) splitOut[i] = i % VTMHIP_GEO_MAX_CAND < numCand ? ( unsigned long long ) sadL[i] : GEO_NO_COST;
  // ---- the filter ----
  {
    const double best = geoBestWholeCost( whole, numCand, lambda );
    const int    pairs = geoNumPairs( numCand );
    for( int t = lane; t < GEO_NUM_SPLIT * pairs; t += THREADS )
    {
      const int s = t / pairs, p = t - s * pairs;
      int       a, b;
      geoPair( p, a, b );
      double cost;
      if( geoComboCost( geoSideCost( sadL[s * VTMHIP_GEO_MAX_CAND + a], a, lambda ), geoSideCost( ( uint64_t ) ( sadW[b] - sadL[s * VTMHIP_GEO_MAX_CAND + b] ), b, lambda ), best, lambda,
                        cost ) )
      {
        const int pos = atomicAdd( &cnt[0], 1 );   // below GEO_MAX_COMBOS < GEO_LIST_CAP
        key[pos] = geoCostBits( cost );
        idx[pos] = ( unsigned short ) geoOrderOf( s, p );
      }
    }
  }
  block_sync<THREADS>();
  const int numPassed = uni( cnt[0] ), numTested = min( numPassed, ( int ) VTMHIP_GEO_MAX_TRY );
  // ---- the ordered list: a bitonic sort over the next power of two ----
  if( numPassed > 1 )
  {
    int M = 2;
    while( M < numPassed ) M <<= 1;
    for( int i = numPassed + lane; i < M; i += THREADS ) { key[i] = GEO_NO_COST; idx[i] = 0xffff; }
    block_sync<THREADS>();
    for( int k = 2; k <= M; k <<= 1 )
      for( int jj = k >> 1; jj > 0; jj >>= 1 )
      {
        for( int i = lane; i < M; i += THREADS )
        {
          const int o = i ^ jj;
          if( o > i )
          {
            const unsigned long long ka = key[i], kb = key[o];
            const int                ia = idx[i], ib = idx[o];
            const bool               swap = ( i & k ) == 0 ? geoComboBefore( kb, ib, ka, ia ) : geoComboBefore( ka, ia, kb, ib );
            if( swap ) { key[i] = kb; key[o] = ka; idx[i] = ( unsigned short ) ib; idx[o] = ( unsigned short ) ia; }
          }
        }
        block_sync<THREADS>();
      }
  }
  if( lane == 0 ) { out.numPassed = numPassed; out.numTested = numTested; }
  for( int r = lane; r < VTMHIP_GEO_MAX_TRY; r += THREADS )
  {
    if( r < numTested )
    {
      int a, b;
      geoPair( idx[r] & 31, a, b );
      unsigned long long *p = reinterpret_cast<unsigned long long *>( &out.combo[r] );
      p[0] = key[r]; p[2] = ( unsigned ) ( idx[r] >> 5 ) | ( ( unsigned ) a << 8 ) | ( ( unsigned ) b << 16 );   // the dist follows below
    }
    else geo_store_combo( &out.combo[r], 0, GEO_NO_COST, 0, 0, 0 );
  }
  // ---- per listed combination: blend and distortion ----
  for( int r = 0; r < numTested; r++ )
  {
    const int s = idx[r] >> 5, c0 = line[3 * s], cx = line[3 * s + 1], cy = line[3 * s + 2];
    int       a, b;
    geoPair( idx[r] & 31, a, b );
    block_sync<THREADS>();   // the previous combination's block and cost have been read
    for( int sg = lane; sg < segs; sg += THREADS )
    {
      int v0[8], v1[8];
      load8s( pred + a * A + 8 * sg, v0 );
      load8s( pred + b * A + 8 * sg, v1 );
      const int base = c0 + cx * ( ( 8 * sg ) & ( w - 1 ) ) + cy * ( ( 8 * sg ) >> lgW );
#pragma unroll
      for( int t = 0; t < 8; t++ ) v0[t] = geoBlendSample( geoWeightOfIdx( base + cx * t ), v0[t], v1[t], bd );
      *reinterpret_cast<uint4 *>( tmp + 8 * sg ) = pack8( v0 );
    }
    block_sync<THREADS>();
    unsigned long long cost = block_dist_walk( useSatd ? VTMHIP_DIST_SATD : VTMHIP_DIST_SAD, orgL, w, tmp, w, w, h, 0, lane, THREADS );   // this lane's share
#pragma unroll
    for( int o = 32; o > 0; o >>= 1 ) cost += __shfl_xor( cost, o, 64 );
    if( THREADS == 256 )
    {
      if( threadIdx.x == 0 ) sCost = 0;
      __syncthreads();
      if( ( threadIdx.x & 63 ) == 0 ) atomicAdd( &sCost, cost );
      __syncthreads();
      if( threadIdx.x == 0 ) out.combo[r].dist = sCost;
    }
    else if( lane == 0 ) out.combo[r].dist = cost;
  }
}

template<int THREADS>
int geo_fused_launch( vtmhip_ctx *ctx, const int16_t *d_refBase, const int16_t *d_orgBase, int16_t *d_predBase, const vtmhip_geo_job *d_jobs, int n, int maxWidth,
                      int maxHeight, int useSatd, vtmhip_geo_result *d_result, uint64_t *d_sadSplit )
{
  const size_t lds = geo_lds_bytes( maxWidth, maxHeight );   // 87.2 KB at most
  // above 64 KB the kernel's limit is raised, once per device and instantiation and to the largest size the entry can ask for: no later call, captured or
  // not, makes anything but its launch
  static std::atomic<bool> raised[GEO_MAX_DEVICES];
  if( lds > 64 * 1024 && ( ctx->device < 0 || ctx->device >= GEO_MAX_DEVICES || !raised[ctx->device].load() ) )
  {
    VTMHIP_HIP( ctx, hipFuncSetAttribute( reinterpret_cast<const void *>( geo_fused_kernel<THREADS> ), hipFuncAttributeMaxDynamicSharedMemorySize,
                                          ( int ) geo_lds_bytes( 64, 64 ) ) );
    if( ctx->device >= 0 && ctx->device < GEO_MAX_DEVICES ) raised[ctx->device].store( true );
  }
  hipLaunchKernelGGL( ( geo_fused_kernel<THREADS> ), dim3( n ), dim3( THREADS ), lds, ctx->stream, d_refBase, d_orgBase, d_predBase, d_jobs, n, maxWidth, maxHeight, useSatd,
                      d_result, ( unsigned long long * ) d_sadSplit );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

// ---- the blend alone ------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__( 256 ) void geo_blend_kernel( const int16_t *srcBase, int16_t *dstBase, const vtmhip_geo_cu_blend_job *__restrict__ jobs, int n )
{
  const int job = ( int ) blockIdx.x * 4 + ( int ) threadIdx.x / 64, lane = ( int ) threadIdx.x & 63;
  if( job >= n ) return;
  const vtmhip_geo_cu_blend_job J = jobs[job];
  if( !geoBlendJobOk( J ) ) return;
  const int      bw = J.width >> J.chroma, bh = J.height >> J.chroma, lgW = 31 - __clz( bw ), bd = J.bitDepth;
  const GeoLine  l  = geoLine( J.splitDir, J.width, J.height, J.chroma, J.chroma );
  const int16_t *s0 = srcBase + J.src0Off, *s1 = srcBase + J.src1Off;
  int16_t       *d  = dstBase + J.dstOff;
  for( int i = lane; i < bw * bh; i += 64 )
  {
    const int x = i & ( bw - 1 ), y = i >> lgW;
    d[( long ) y * J.dstStride + x] = ( int16_t ) geoBlendSample( geoWeightOfIdx( geoLineIdx( l, x, y ) ), s0[( long ) y * J.src0Stride + x], s1[( long ) y * J.src1Stride + x], bd );
  }
}

}   // namespace

extern "C"
{

int vtmhip_geo_struct_size( int which )
{
  switch( which )
  {
  case 0: return ( int ) sizeof( vtmhip_geo_job );
  case 1: return ( int ) sizeof( vtmhip_geo_cand );
  case 2: return ( int ) sizeof( vtmhip_geo_combo );
  case 3: return ( int ) sizeof( vtmhip_geo_result );
  case 4: return ( int ) sizeof( vtmhip_geo_cu_blend_job );
  default: return -1;
  }
}

int vtmhip_geo_lanes_per_job( int maxWidth, int maxHeight )
{
  if( !geoSizeOk( maxWidth, maxHeight ) ) return 0;
  return maxWidth * maxHeight <= 1024 ? 64 : 256;
}

int vtmhip_geo_tables_host( int splitDir, int width, int height, int chroma, int16_t *weightOut, int16_t *maskOut )
{
  return geoHostTables( splitDir, width, height, chroma, weightOut, maskOut ) ? VTMHIP_E_INVALID : VTMHIP_OK;
}

int vtmhip_geo_host( const vtmhip_geo_job *job, const int16_t *orgBase, const int16_t *const pred[VTMHIP_GEO_MAX_CAND], int useSatd, vtmhip_geo_result *result,
                     uint64_t *sadSplit, int16_t *blend )
{
  return geoHostJob( job, orgBase, pred, useSatd, result, sadSplit, blend ) ? VTMHIP_E_INVALID : VTMHIP_OK;
}

int vtmhip_geo_cand_satd_batch_dev( vtmhip_ctx *ctx, const int16_t *d_refBase, const int16_t *d_orgBase, int16_t *d_predBase, const vtmhip_geo_job *d_jobs, int n,
                                    int maxWidth, int maxHeight, int useSatd, vtmhip_geo_result *d_result, uint64_t *d_sadSplit )
{
  VTMHIP_BATCH_ENTRY( ctx, n, d_refBase && d_orgBase && d_jobs && d_result );
  const int lanes = vtmhip_geo_lanes_per_job( maxWidth, maxHeight );
  VTMHIP_REQUIRE( ctx, lanes != 0, "maxWidth / maxHeight: a GEO size (sides 8 .. 64, w < 8h, h < 8w)" );
  VTMHIP_TIME_KERNEL( ctx, "geo_fused_kernel" );
  if( lanes == 256 ) return geo_fused_launch<256>( ctx, d_refBase, d_orgBase, d_predBase, d_jobs, n, maxWidth, maxHeight, useSatd, d_result, d_sadSplit );
  return geo_fused_launch<64>( ctx, d_refBase, d_orgBase, d_predBase, d_jobs, n, maxWidth, maxHeight, useSatd, d_result, d_sadSplit );
}

int vtmhip_geo_blend_batch_dev( vtmhip_ctx *ctx, const int16_t *d_srcBase, int16_t *d_dstBase, const vtmhip_geo_cu_blend_job *d_jobs, int n )
{
  VTMHIP_BATCH_ENTRY( ctx, n, d_srcBase && d_dstBase && d_jobs );
  VTMHIP_TIME_KERNEL( ctx, "geo_blend_kernel" );
  hipLaunchKernelGGL( geo_blend_kernel, dim3( ( n + 3 ) / 4 ), dim3( 256 ), 0, ctx->stream, d_srcBase, d_dstBase, d_jobs, n );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

}   // extern "C"
