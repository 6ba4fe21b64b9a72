// ciip.hip -- the CIIP candidates of the merge pre-selection (EncCu::xCheckRDCostMerge2Nx2N, EncCu.cpp:2460-2523; hook B10) and the RD stage's blend (:2706-2735).
//   vtmhip_set_lmcs_inv_lut           the reshaper's inverse LUT of a context (a slot of its own, beside the forward LUT of lmcs.hip)
//   vtmhip_ciip_cand_satd_batch_dev   per CU the planar block once and, per candidate, inter block -> forward LUT -> blend -> optional kept store -> inverse LUT ->
//                                     SATD / SAD against the original: the costs and the kept blocks are all that is stored
//   vtmhip_ciip_blend_batch_dev       IntraPrediction::geneWeightedPred in place, luma and 4:2:0 chroma blocks
//   vtmhip_ciip_host / vtmhip_ciip_blend_host   the same as host arithmetic (ciip_host.hpp)
// The rules are ciip_rules.hpp's (planar, the line filter and PDPC through intra_rules.hpp); the motion compensation is mc_any (mc_block.hpp) with the LDS sinks of
// mc_sinks.hpp, the distortion block_dist_walk (dist_block.hpp; the tile rule is had.hpp's had_tile_shape).
//
// ciip_fused_kernel<THREADS, JPB>: THREADS lanes per CU and JPB CUs per workgroup as mmvd_fused_kernel -- <8, 8>, <16, 4>, <64, 1>, <256, 1> by
// vtmhip_mc_lanes_per_block( maxWidth, maxHeight ).  A lane group checks its job (ciipJobOk; a malformed job leaves four UINT64_MAX and nothing else), loads the
// original block into LDS and the two unfiltered lines into the H-pass scratch, forms the [1 2 1] lines and from them the planar block with PDPC, once; then per
// candidate: mc_any with the ToLds sink (and the default-weight AvgOver sink for list 1 of a bi candidate) or a copy of the given block, one pass of 8-sample
// segments -- forward LUT, blend against the planar block, the kept store, inverse LUT -- and block_dist_walk straight from LDS.  Neither the table nor a cursor is
// read back, so the entry only queues one launch.
// LDS per lane group, in samples: original + planar + prediction (3 x maxW x maxH), the lines (2 x 136), the H-pass scratch (maxW x (maxH + 7)); per workgroup:
//   <8, 8>     8 x 8     8 x  584 x 2 B =  9.1 KB          <64, 1>    32 x 32    4 592 x 2 B =  9.0 KB
//   <16, 4>   16 x 16    4 x 1408 x 2 B = 11.0 KB          <256, 1>   64 x 64   17 104 x 2 B = 33.4 KB (four workgroups of a CU's 160 KB: 4 waves per SIMD)
// Registers, scratch and waves per SIMD of every instantiation: profiles/ciip_kernel_resources.txt.
//
// ciip_blend_kernel: 256 threads, L = 16 / 64 / 256 lanes per job by the largest well-formed block of the table (intra_lane_rule.hpp; ciip_shape_kernel leaves L in
// the stream's workspace), intra_chunk( L ) consecutive jobs per workgroup.  A lane group stages the lines it predicts from (filtered for luma) in LDS and then, per
// sample: planar with PDPC, the forward LUT on the inter sample where asked, the blend, the store over the inter sample.  LDS: 16 x 272 x 2 B = 8.5 KB.
#include "ctx.hpp"
#include "mc_block.hpp"
#include "mc_sinks.hpp"
#include "dist_block.hpp"
#include "intra_lane_rule.hpp"
#include "ciip_rules.hpp"
#include "ciip_host.hpp"   // the host entries' bodies: shared with host/test_ciip.cpp

namespace
{

constexpr unsigned long long CIIP_NO_COST = ~0ull;

__host__ __device__ inline int ciip_group_samples( int maxW, int maxH ) { return ( 3 * maxW * maxH + 2 * CIIP_LINE + maxW * ( maxH + 7 ) + 7 ) & ~7; }

template<int THREADS, int JPB>
__global__ __launch_bounds__( THREADS * JPB ) void ciip_fused_kernel( const int16_t *__restrict__ refBase, const int16_t *__restrict__ lineBase, const int16_t *__restrict__ orgBase,
                                                                      int16_t *predBase, const vtmhip_ciip_job *__restrict__ jobs, int n, int maxW, int maxH, int useSatd,
                                                                      int lutDepth, const int16_t *__restrict__ fwd, const int16_t *__restrict__ inv,
                                                                      unsigned long long *__restrict__ distOut )
{
  extern __shared__ __attribute__( ( aligned( 16 ) ) ) int16_t lds[];
  __shared__ unsigned long long sCost;   // THREADS == 256: the block's cost
  const int sub  = JPB > 1 ? ( int ) threadIdx.x / THREADS : 0;
  const int lane = JPB > 1 ? ( int ) threadIdx.x % THREADS : ( int ) threadIdx.x;
  const int item = xcd_order( ( int ) blockIdx.x, ( int ) gridDim.x ) * JPB + sub;
  if( item >= n ) return;
  const vtmhip_ciip_job &j = jobs[item];
  unsigned long long    *out = distOut + 4L * item;
  bool ok = ciipJobOk( j, maxW, maxH, lutDepth );
  if( ok && !predBase )
    for( int k = 0; k < j.numCand; k++ ) ok = ok && j.cand[k].mode != CIIP_MODE_GIVEN && j.cand[k].keepOff < 0;
  if( !ok )   // uniform over the lane group (and over the workgroup where it is one group)
  {
    if( lane < VTMHIP_CIIP_MAX_CAND ) out[lane] = CIIP_NO_COST;
    return;
  }
  const int w = j.width, h = j.height, bd = j.bitDepth, lgW = 31 - __clz( w ), area = w * h, maxVal = ( 1 << bd ) - 1, nLine = 2 * w + 2 * h + 2;
  int16_t  *orgL = lds + sub * ciip_group_samples( maxW, maxH ), *plan = orgL + maxW * maxH, *pred = plan + maxW * maxH, *line = pred + maxW * maxH, *tmp = line + 2 * CIIP_LINE;
  {
    const int16_t *org = orgBase + j.orgOff, *ln = lineBase + j.lineOff;
    for( int i = lane; i < area; i += THREADS ) orgL[i] = org[( long ) ( i >> lgW ) * j.orgStride + ( i & ( w - 1 ) )];
    for( int i = lane; i < nLine; i += THREADS ) tmp[i] = ln[i];   // nLine <= maxW * ( maxH + 7 ) for every CIIP size
  }
  block_sync<THREADS>();
  vtmhip_intra_params p;
  ciipIntraParams( w, h, false, p );
  for( int i = lane; i < nLine; i += THREADS ) line[i] = ciipLineSample( tmp, w, h, i, p.refFilterFlag );
  block_sync<THREADS>();
  {
    const IntraBlk b = ciipIntraBlk( line, line + 2 * w + 1, w, h, bd );
    for( int i = lane; i < area; i += THREADS ) plan[i] = ( int16_t ) ciipIntraSample( p, b, i & ( w - 1 ), i >> lgW, false );
  }
  const int wIntra = ciipWeightIntra( j.leftIntra, j.aboveIntra ), numCand = j.numCand, lmcs = j.lmcs;
  if( lane >= numCand && lane < VTMHIP_CIIP_MAX_CAND ) out[lane] = CIIP_NO_COST;

  for( int k = 0; k < numCand; k++ )
  {
    const vtmhip_ciip_cand &c = j.cand[k];
    block_sync<THREADS>();   // the planar block is in place; the previous candidate's block and cost have been read
    if( c.mode == CIIP_MODE_GIVEN )
    {
      const int16_t *src = predBase + c.srcOff;
      for( int i = lane; i < area; i += THREADS ) pred[i] = src[( long ) ( i >> lgW ) * c.srcStride + ( i & ( w - 1 ) )];
    }
    else
    {
      vtmhip_mc_job m;
      m.width = ( int16_t ) w; m.height = ( int16_t ) h; m.bitDepth = ( uint8_t ) bd; m.useAltHpelIf = c.useAltHpelIf; m.chroma = 0; m.dstOff = 0; m.dstStride = 0;
      const int l = c.mode == CIIP_MODE_L1;   // the first (or only) list
      m.bi = c.mode == CIIP_MODE_BI;
      m.refOff = c.refOff[l]; m.refStride = c.refStride[l]; m.mvHor = c.mv[l][0]; m.mvVer = c.mv[l][1];
      mc_any<THREADS>( m, refBase, tmp, lane, ToLds{ pred, w } );
      if( c.mode == CIIP_MODE_BI )
      {
        block_sync<THREADS>();
        m.refOff = c.refOff[1]; m.refStride = c.refStride[1]; m.mvHor = c.mv[1][0]; m.mvVer = c.mv[1][1];
        mc_any<THREADS>( m, refBase, tmp, lane, AvgOver{ pred, w, max( 2, 14 - bd ) + 1, maxVal, AVG_BCW_DEFAULT } );
      }
    }
    block_sync<THREADS>();
    int16_t *keep = c.keepOff >= 0 ? predBase + c.keepOff : nullptr;
    for( int s = lane; s < ( area >> 3 ); s += THREADS )   // area is a multiple of 64
    {
      int v[8], q[8];
      load8s( pred + 8 * s, v );
      load8s( plan + 8 * s, q );
#pragma unroll
      for( int t = 0; t < 8; t++ ) v[t] = ciipBlendSample( lmcs ? ciipLutAt( fwd, v[t], maxVal ) : v[t], q[t], wIntra );
      if( keep ) store8g( keep + 8 * s, v );
      if( lmcs )
      {
#pragma unroll
        for( int t = 0; t < 8; t++ ) v[t] = ciipLutAt( inv, v[t], maxVal );
      }
      *reinterpret_cast<uint4 *>( pred + 8 * s ) = pack8( v );
    }
    block_sync<THREADS>();
    unsigned long long cost = block_dist_walk( useSatd ? VTMHIP_DIST_SATD : VTMHIP_DIST_SAD, orgL, w, pred, w, w, h, 0, lane, THREADS );   // this lane's share
#pragma unroll
    for( int o = ( THREADS < 64 ? THREADS : 64 ) >> 1; o > 0; o >>= 1 ) cost += __shfl_xor( cost, o, 64 );
    if( THREADS == 256 )
    {
      if( threadIdx.x == 0 ) sCost = 0;
      __syncthreads();
      if( ( threadIdx.x & 63 ) == 0 ) atomicAdd( &sCost, cost );
      __syncthreads();
      if( threadIdx.x == 0 ) out[k] = sCost;
    }
    else if( lane == 0 ) out[k] = cost;
  }
}

template<int THREADS, int JPB>
int ciip_fused_launch( vtmhip_ctx *ctx, const int16_t *d_refBase, const int16_t *d_lineBase, const int16_t *d_orgBase, int16_t *d_predBase, const vtmhip_ciip_job *d_jobs, int n,
                       int maxWidth, int maxHeight, int useSatd, int lutDepth, uint64_t *d_dist )
{
  const size_t lds = ( size_t ) JPB * ciip_group_samples( maxWidth, maxHeight ) * sizeof( int16_t );   // 33.4 KB at most
  hipLaunchKernelGGL( ( ciip_fused_kernel<THREADS, JPB> ), dim3( ( n + JPB - 1 ) / JPB ), dim3( THREADS * JPB ), lds, ctx->stream, d_refBase, d_lineBase, d_orgBase, d_predBase,
                      d_jobs, n, maxWidth, maxHeight, useSatd, lutDepth, ( const int16_t * ) ctx->lmcsFwd, ( const int16_t * ) ctx->lmcsInv, ( unsigned long long * ) d_dist );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

// ---- the blend alone ------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__( 256 ) void ciip_shape_kernel( const vtmhip_ciip_blend_job *__restrict__ jobs, int n, int fwdDepth, int *__restrict__ lanes )
{
  __shared__ int sMax;
  if( threadIdx.x == 0 ) sMax = 16;
  __syncthreads();
  int m = 0;
  for( int i = threadIdx.x; i < n; i += 256 )
  {
    const vtmhip_ciip_blend_job b = jobs[i];
    if( ciipBlendJobOk( b, fwdDepth ) ) m = max( m, b.width * b.height );
  }
  if( m ) atomicMax( &sMax, m );
  __syncthreads();
  if( threadIdx.x == 0 ) *lanes = intra_lanes( sMax );
}

template<int L>
__device__ __forceinline__ void ciip_blend_body( int16_t *sLine, const int16_t *__restrict__ lineBase, int16_t *predBase, const vtmhip_ciip_blend_job *__restrict__ jobs, int n,
                                                 const int16_t *__restrict__ fwd, int fwdDepth )
{
  constexpr int G = 256 / L, CHUNK = L == 16 ? 16 : L == 64 ? 8 : 4;
  const int tid = threadIdx.x, g = tid / L, l = tid % L;
  const int jBegin = blockIdx.x * CHUNK, jEnd = min( n, jBegin + CHUNK );
  int16_t  *line = sLine + g * 2 * CIIP_LINE;
  for( int base = jBegin; base < jEnd; base += G )
  {
    const int job = base + g;
    bool      ok  = job < jEnd;
    vtmhip_ciip_blend_job J;
    if( ok )
    {
      J  = jobs[job];
      ok = ciipBlendJobOk( J, fwdDepth ) && J.width * J.height <= ( L == 16 ? 64 : L == 64 ? 1024 : INTRA_MAX_AREA );   // the second part cannot happen: L comes from the largest block
    }
    const int w = ok ? J.width : 4, h = ok ? J.height : 4, lgW = 31 - __clz( w ), chroma = ok ? J.chroma : 0;
    vtmhip_intra_params p;
    ciipIntraParams( w, h, chroma != 0, p );
    block_sync<L>();   // the previous round's readers are done
    if( ok )
    {
      const int16_t *ln = lineBase + J.lineOff;
      for( int i = l; i < 2 * w + 2 * h + 2; i += L ) line[i] = ciipLineSample( ln, w, h, i, p.refFilterFlag );
    }
    block_sync<L>();
    if( ok )
    {
      const IntraBlk b = ciipIntraBlk( line, line + 2 * w + 1, w, h, J.bitDepth );
      const int      wIntra = ciipWeightIntra( J.leftIntra, J.aboveIntra ), maxVal = ( 1 << J.bitDepth ) - 1;
      int16_t       *pred = predBase + J.predOff;
      for( int i = l; i < w * h; i += L )
      {
        const int x = i & ( w - 1 ), y = i >> lgW;
        int16_t  *at = pred + ( long ) y * J.predStride + x;
        const int v  = J.mapFwd ? ciipLutAt( fwd, *at, maxVal ) : *at;
        *at = ( int16_t ) ciipBlendSample( v, ciipIntraSample( p, b, x, y, chroma != 0 ), wIntra );
      }
    }
  }
}

__global__ __launch_bounds__( 256 ) void ciip_blend_kernel( const int *__restrict__ lanesPtr, const int16_t *__restrict__ lineBase, int16_t *predBase,
                                                            const vtmhip_ciip_blend_job *__restrict__ jobs, int n, const int16_t *__restrict__ fwd, int fwdDepth )
{
  __shared__ int16_t sLine[16 * 2 * CIIP_LINE];
  const int lanes = uni( *lanesPtr );
  if( ( long ) blockIdx.x * intra_chunk( lanes ) >= n ) return;
  if( lanes == 16 ) ciip_blend_body<16>( sLine, lineBase, predBase, jobs, n, fwd, fwdDepth );
  else if( lanes == 64 ) ciip_blend_body<64>( sLine, lineBase, predBase, jobs, n, fwd, fwdDepth );
  else ciip_blend_body<256>( sLine, lineBase, predBase, jobs, n, fwd, fwdDepth );
}

}   // namespace

extern "C"
{

int vtmhip_ciip_struct_size( int which )
{
  switch( which )
  {
  case 0: return ( int ) sizeof( vtmhip_ciip_job );
  case 1: return ( int ) sizeof( vtmhip_ciip_cand );
  case 2: return ( int ) sizeof( vtmhip_ciip_blend_job );
  default: return -1;
  }
}

int vtmhip_set_lmcs_inv_lut( vtmhip_ctx *ctx, const int16_t *invLut, int lumaBD )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, invLut != nullptr, "null inverse LUT" );
  VTMHIP_REQUIRE( ctx, lumaBD >= 8 && lumaBD <= 12, "lumaBD must be 8..12" );
  std::lock_guard<std::mutex> lock( ctx->initMutex );
  if( !ctx->lmcsInv ) VTMHIP_HIP( ctx, hipMalloc( ( void ** ) &ctx->lmcsInv, ( ( size_t ) 1 << 12 ) * sizeof( int16_t ) ) );
  VTMHIP_HIP( ctx, hipMemcpyAsync( ctx->lmcsInv, invLut, ( ( size_t ) 1 << lumaBD ) * sizeof( int16_t ), hipMemcpyHostToDevice, ctx->stream ) );
  VTMHIP_HIP( ctx, hipStreamSynchronize( ctx->stream ) );   // the caller's array may go away
  ctx->lmcsInvBD = lumaBD;
  return VTMHIP_OK;
}

int vtmhip_ciip_host( const vtmhip_ciip_job *job, const int16_t *lineBase, const int16_t *orgBase, const int16_t *const inter[VTMHIP_CIIP_MAX_CAND], const int16_t *fwdLut,
                      const int16_t *invLut, int16_t *blend, uint64_t satd[VTMHIP_CIIP_MAX_CAND], uint64_t sad[VTMHIP_CIIP_MAX_CAND] )
{
  return ciipHostJob( job, lineBase, orgBase, inter, fwdLut, invLut, blend, satd, sad ) ? VTMHIP_E_INVALID : VTMHIP_OK;
}

int vtmhip_ciip_blend_host( const vtmhip_ciip_blend_job *job, const int16_t *lineBase, int16_t *predBase, const int16_t *fwdLut )
{
  return ciipHostBlendJob( job, lineBase, predBase, fwdLut ) ? VTMHIP_E_INVALID : VTMHIP_OK;
}

int vtmhip_ciip_cand_satd_batch_dev( vtmhip_ctx *ctx, const int16_t *d_refBase, const int16_t *d_lineBase, const int16_t *d_orgBase, int16_t *d_predBase,
                                     const vtmhip_ciip_job *d_jobs, int n, int maxWidth, int maxHeight, int useSatd, int lmcs, uint64_t *d_dist )
{
  VTMHIP_BATCH_ENTRY( ctx, n, d_refBase && d_lineBase && d_orgBase && d_jobs && d_dist );
  const int lanes = vtmhip_mc_lanes_per_block( maxWidth, maxHeight );
  VTMHIP_REQUIRE( ctx, lanes != 0 && ciipSizeOk( maxWidth, maxHeight ), "maxWidth / maxHeight: a CIIP size (sides 4 .. 64, at least 64 samples)" );
  int lutDepth = 0;
  if( lmcs )
  {
    VTMHIP_REQUIRE( ctx, ctx->lmcsLumaBD != 0 && ctx->lmcsInvBD != 0, "lmcs: vtmhip_set_lmcs_fwd_lut / vtmhip_set_lmcs_inv_lut have not both been called" );
    VTMHIP_REQUIRE( ctx, ctx->lmcsLumaBD == ctx->lmcsInvBD, "lmcs: the forward and the inverse LUT have different depths" );
    lutDepth = ctx->lmcsLumaBD;
  }
  VTMHIP_TIME_KERNEL( ctx, "ciip_fused_kernel" );
  if( lanes == 256 ) return ciip_fused_launch<256, 1>( ctx, d_refBase, d_lineBase, d_orgBase, d_predBase, d_jobs, n, maxWidth, maxHeight, useSatd, lutDepth, d_dist );
  if( lanes == 64 ) return ciip_fused_launch<64, 1>( ctx, d_refBase, d_lineBase, d_orgBase, d_predBase, d_jobs, n, maxWidth, maxHeight, useSatd, lutDepth, d_dist );
  if( lanes == 16 ) return ciip_fused_launch<16, 4>( ctx, d_refBase, d_lineBase, d_orgBase, d_predBase, d_jobs, n, maxWidth, maxHeight, useSatd, lutDepth, d_dist );
  return ciip_fused_launch<8, 8>( ctx, d_refBase, d_lineBase, d_orgBase, d_predBase, d_jobs, n, maxWidth, maxHeight, useSatd, lutDepth, d_dist );
}

int vtmhip_ciip_blend_batch_dev( vtmhip_ctx *ctx, const int16_t *d_lineBase, int16_t *d_predBase, const vtmhip_ciip_blend_job *d_jobs, int n )
{
  VTMHIP_BATCH_ENTRY( ctx, n, d_lineBase && d_predBase && d_jobs );
  void *arena = nullptr;
  VTMHIP_TRY( vtmhip_internal_workspace( ctx, 256, &arena ) );
  int *d_lanes = ( int * ) arena;
  hipLaunchKernelGGL( ciip_shape_kernel, dim3( 1 ), dim3( 256 ), 0, ctx->stream, d_jobs, n, ctx->lmcsLumaBD, d_lanes );
  VTMHIP_LAUNCHED( ctx );
  VTMHIP_TIME_KERNEL( ctx, "ciip_blend_kernel" );
  hipLaunchKernelGGL( ciip_blend_kernel, dim3( ( n + INTRA_MIN_CHUNK - 1 ) / INTRA_MIN_CHUNK ), dim3( 256 ), 0, ctx->stream, d_lanes, d_lineBase, d_predBase, d_jobs, n,
                      ( const int16_t * ) ctx->lmcsFwd, ctx->lmcsLumaBD );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

}   // extern "C"
