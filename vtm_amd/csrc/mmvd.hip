// mmvd.hip -- the MMVD candidates of the merge pre-selection (EncCu::xCheckRDCostMerge2Nx2N, EncCu.cpp:2524-2562; hook B10).
//   vtmhip_mmvd_cand_satd_batch_dev   per CU the 64 candidates of MergeCtx::setMmvdMergeCandiInfo (mmvd_rules.hpp), their luma predictions and the SATD / SAD against
//                                     the original: the candidate records and the costs are all that is stored
//   vtmhip_mmvd_cands_host            the derivation as host arithmetic
// Two routes to the same tables:
//   fused             mmvd_fused_kernel: a lane group (vtmhip_mc_lanes_per_block lanes) takes a slice of one CU's candidates.  It loads the original block into LDS
//                     once and, per plain candidate, derives the motion, runs mc_block per list with a sink into LDS (clipped samples for a uni candidate; the list-0
//                     14-bit block, then the average written over it for a bi one) and reduces the block to its cost by block_dist_walk (dist_block.hpp; the tile rule is had.hpp's had_tile_shape) straight from LDS.  The BDOF
//                     candidates (at most 24 per CU) are expanded into vtmhip_pred_job rows and predictions in a workspace: vtmhip_bdof_batch_dev, the distortion
//                     call, and a scatter of the costs to the candidates' slots.
//   VTMHIP_MMVD_FUSED=0   every candidate is expanded: vtmhip_motion_compensation_batch_dev (uni, addAvg), vtmhip_mc_batch_dev + vtmhip_add_weighted_avg_batch_dev
//                     (a BCW weight), vtmhip_bdof_batch_dev, then the distortion call and the scatter.
// Unset, the switch leaves the fused kernel to the batches of up to a wave per block and the expansion to the larger ones (the measurements are in DESIGN.md 4.19).
// The host reads the job table back, checks it (mmvdJobOk) and counts the rows of every class from it, so the expansion's cursors are never read back.
#include "ctx.hpp"
#include "stage.hpp"
#include "mc_block.hpp"
#include "mc_sinks.hpp"   // ToLds, AvgOver: shared with ciip.hip
#include "mv_rules.hpp"
#include "dist_block.hpp"
#include "mmvd_rules.hpp"

// the host / device restatement of clipMvInPic against the device's definition
static_assert( mmvdClipMax( 416, 24 ) == MVR_CLIP_MAX( 416, 24 ) && mmvdClipMax( 3840, 3832 ) == MVR_CLIP_MAX( 3840, 3832 ), "mmvd_rules.hpp: clipMvInPic maximum" );
static_assert( ( int ) AVG_BCW_DEFAULT == ( int ) MMVD_BCW_DEFAULT, "mc_sinks.hpp: the weight that means addAvg" );
static_assert( mmvdClipMin( 128, 0 ) == -( ( 128 + 8 - 1 ) << 4 ) && mmvdClipMin( 64, 200 ) == -( ( 64 + 8 + 200 - 1 ) << 4 ), "mmvd_rules.hpp: clipMvInPic minimum" );

namespace
{

constexpr unsigned long long MMVD_NO_COST = ~0ull;

// LDS of one lane group, in samples: the original block (orgInLds: the groups of up to a wave; a workgroup per block reads it from global memory, so that two
// 128 x 128 workgroups fit a CU), the prediction, the H-pass intermediates of mc_block
__host__ __device__ inline int mmvd_group_samples( int maxW, int maxH, bool orgInLds ) { return ( ( orgInLds ? 2 : 1 ) * maxW * maxH + maxW * ( maxH + 7 ) + 7 ) & ~7; }

// THREADS lanes per group and JPB groups per workgroup as motion_comp_kernel (mc.hip); an item is (job, slice): `cpi` consecutive candidates of one CU
template<int THREADS, int JPB>
__global__ __launch_bounds__( THREADS * JPB ) void mmvd_fused_kernel( vtmhip_pic_params pic, const int16_t *__restrict__ orgBase, const int16_t *__restrict__ refBase,
                                                                      const vtmhip_mmvd_job *__restrict__ jobs, int items, int cpi, int maxW, int maxH, int useSatd,
                                                                      vtmhip_mmvd_cand *__restrict__ candOut, unsigned long long *__restrict__ distOut )
{
  extern __shared__ __attribute__( ( aligned( 16 ) ) ) int16_t lds[];
  __shared__ unsigned long long sCost;   // THREADS == 256: the block's cost
  const int sub  = JPB > 1 ? ( int ) threadIdx.x / THREADS : 0;
  const int lane = JPB > 1 ? ( int ) threadIdx.x % THREADS : ( int ) threadIdx.x;
  const int item = xcd_order( ( int ) blockIdx.x, ( int ) gridDim.x ) * JPB + sub;
  if( item >= items ) return;
  constexpr bool ORG_LDS = THREADS <= 64;
  int16_t  *orgL = lds + sub * mmvd_group_samples( maxW, maxH, ORG_LDS ), *pred = ORG_LDS ? orgL + maxW * maxH : orgL, *tmp = pred + maxW * maxH;
  const int slices = VTMHIP_MMVD_NUM_CAND / cpi, jobIdx = item / slices, first = ( item % slices ) * cpi;
  const vtmhip_mmvd_job &j = jobs[jobIdx];
  const int w = j.width, h = j.height, lgW = 31 - __clz( w );
  const int16_t *org = orgBase + j.orgOff;
  int            os  = j.orgStride;
  if( ORG_LDS )
  {
    for( int i = lane; i < w * h; i += THREADS ) orgL[i] = org[( long ) ( i >> lgW ) * os + ( i & ( w - 1 ) )];
    org = orgL; os = w;
  }
  for( int k = 0; k < cpi; k++ )
  {
    const int        cand = first + k, slot = jobIdx * VTMHIP_MMVD_NUM_CAND + cand;
    vtmhip_mmvd_cand rec;
    int              mode;
    int32_t          pmv[2][2];
    mmvdDerive( j, pic.picW, pic.picH, pic.ctuSize, cand, rec, mode, pmv );
    if( lane == 0 )
    {
      candOut[slot] = rec;
      if( rec.kind == VTMHIP_MMVD_NOT_TESTED ) distOut[slot] = MMVD_NO_COST;
    }
    if( rec.kind != VTMHIP_MMVD_PLAIN ) continue;   // BDOF: the expansion's
    const vtmhip_mmvd_base &s = j.base[mmvdBase( cand )];
    vtmhip_mc_job m;
    m.width = ( int16_t ) w; m.height = ( int16_t ) h; m.bitDepth = j.bitDepth; m.useAltHpelIf = rec.useAltHpelIf; m.chroma = 0; m.dstOff = 0; m.dstStride = 0;
    const int l = mode == MMVD_PRED_L1;   // the first (or only) list
    m.bi = mode == MMVD_PRED_BI;
    m.refOff = l ? s.refOff[1] : s.refOff[0]; m.refStride = l ? s.refStride[1] : s.refStride[0];
    m.mvHor = l ? pmv[1][0] : pmv[0][0]; m.mvVer = l ? pmv[1][1] : pmv[0][1];
    block_sync<THREADS>();   // the original is in place; the previous candidate's cost has been read
    mc_any<THREADS>( m, refBase, tmp, lane, ToLds{ pred, w } );
    block_sync<THREADS>();
    if( mode == MMVD_PRED_BI )
    {
      const int headRoom = max( 2, 14 - ( int ) j.bitDepth );
      m.refOff = s.refOff[1]; m.refStride = s.refStride[1]; m.mvHor = pmv[1][0]; m.mvVer = pmv[1][1];
      mc_any<THREADS>( m, refBase, tmp, lane, AvgOver{ pred, w, headRoom + 1, ( 1 << j.bitDepth ) - 1, rec.bcwWeightL1 } );
      block_sync<THREADS>();
    }
    unsigned long long cost = block_dist_walk( useSatd ? VTMHIP_DIST_SATD : VTMHIP_DIST_SAD, org, os, pred, w, w, h, 0, lane, THREADS );   // this lane's share
#pragma unroll
    for( int o = ( THREADS < 64 ? THREADS : 64 ) >> 1; o > 0; o >>= 1 ) cost += __shfl_xor( cost, o, 64 );
    if( THREADS == 256 )
    {
      if( threadIdx.x == 0 ) sCost = 0;
      __syncthreads();
      if( ( threadIdx.x & 63 ) == 0 ) atomicAdd( &sCost, cost );
      __syncthreads();
      if( threadIdx.x == 0 ) distOut[slot] = sCost;
    }
    else if( lane == 0 ) distOut[slot] = cost;
  }
}

// the tables the expansion writes: a row per expanded candidate (its prediction block, its distortion job, its slot), and per class the job rows of the call that
// predicts it
struct MmvdExpand
{
  int                *cursor;     // [4]: rows, BDOF rows, plain rows, weighted rows
  int                *slot;       // [rows]: job * 64 + cand
  vtmhip_dist_job    *distJobs;   // [rows]
  vtmhip_pred_job    *bdofJobs, *plainJobs;
  vtmhip_mc_job      *mcJobs;     // [2 * weighted]: the two 14-bit blocks of a weighted candidate, inside the intermediates
  vtmhip_pelop_job   *pelJobs;    // [weighted]
  unsigned long long *dist;       // [rows]
};

// all == 0: the BDOF candidates alone (the fused kernel has written the records); all != 0: every candidate, the records and the untested slots' cost as well
__global__ __launch_bounds__( 256 ) void mmvd_expand_kernel( vtmhip_pic_params pic, const vtmhip_mmvd_job *__restrict__ jobs, int n, int area, int useSatd, int all, MmvdExpand e,
                                                            vtmhip_mmvd_cand *__restrict__ candOut, unsigned long long *__restrict__ distOut )
{
  const int at = ( int ) ( blockIdx.x * blockDim.x + threadIdx.x );
  if( at >= n * VTMHIP_MMVD_NUM_CAND ) return;
  const int              jobIdx = at / VTMHIP_MMVD_NUM_CAND, cand = at % VTMHIP_MMVD_NUM_CAND;
  const vtmhip_mmvd_job &j = jobs[jobIdx];
  vtmhip_mmvd_cand       rec;
  int                    mode;
  int32_t                pmv[2][2];
  mmvdDerive( j, pic.picW, pic.picH, pic.ctuSize, cand, rec, mode, pmv );
  if( all )
  {
    candOut[at] = rec;
    if( rec.kind == VTMHIP_MMVD_NOT_TESTED ) distOut[at] = MMVD_NO_COST;
  }
  if( rec.kind == VTMHIP_MMVD_NOT_TESTED || ( !all && rec.kind != VTMHIP_MMVD_BDOF ) ) return;
  const vtmhip_mmvd_base &s = j.base[mmvdBase( cand )];
  const int     row = atomicAdd( &e.cursor[0], 1 );
  const int64_t predOff = ( int64_t ) row * area;
  e.slot[row] = at;
  vtmhip_dist_job d;
  d.orgOff = j.orgOff; d.curOff = predOff; d.orgStride = j.orgStride; d.curStride = j.width; d.width = j.width; d.height = j.height; d.subShift = 0;
  d.kind = ( int16_t ) ( useSatd ? VTMHIP_DIST_SATD : VTMHIP_DIST_SAD );
  e.distJobs[row] = d;
  if( rec.kind == VTMHIP_MMVD_PLAIN && mode == MMVD_PRED_BI && rec.bcwWeightL1 != MMVD_BCW_DEFAULT )
  {
    const int t = atomicAdd( &e.cursor[3], 1 );
    for( int l = 0; l < 2; l++ )
    {
      vtmhip_mc_job m;
      m.refOff = s.refOff[l]; m.dstOff = ( int64_t ) ( 2 * t + l ) * area; m.refStride = s.refStride[l]; m.dstStride = j.width; m.width = j.width; m.height = j.height;
      m.mvHor = pmv[l][0]; m.mvVer = pmv[l][1]; m.bi = 1; m.bitDepth = j.bitDepth; m.useAltHpelIf = rec.useAltHpelIf; m.chroma = 0;
      e.mcJobs[2 * t + l] = m;
    }
    vtmhip_pelop_job p;
    p.aOff = ( int64_t ) ( 2 * t ) * area; p.bOff = ( int64_t ) ( 2 * t + 1 ) * area; p.dstOff = predOff; p.aStride = p.bStride = p.dstStride = j.width;
    p.width = j.width; p.height = j.height; p.bitDepth = j.bitDepth; p.bcwWeight = rec.bcwWeightL1; p.pad1 = p.pad2 = 0; p.pad3 = 0;
    e.pelJobs[t] = p;
    return;
  }
  vtmhip_pred_job p;
  p.orgOff = j.orgOff; p.refOff[0] = s.refOff[0]; p.refOff[1] = s.refOff[1]; p.predOff = predOff; p.outOff = 0;
  p.orgStride = j.orgStride; p.refStride[0] = s.refStride[0]; p.refStride[1] = s.refStride[1]; p.predStride = j.width; p.outStride = 0;
  p.mv[0][0] = pmv[0][0]; p.mv[0][1] = pmv[0][1]; p.mv[1][0] = pmv[1][0]; p.mv[1][1] = pmv[1][1];
  p.width = j.width; p.height = j.height; p.mode = ( uint8_t ) mode; p.epilogue = 0; p.bitDepth = j.bitDepth; p.useAltHpelIf = rec.useAltHpelIf; p.chroma = 0; p.route = 0;
  p.bcwWeight = 0;
  if( rec.kind == VTMHIP_MMVD_BDOF ) e.bdofJobs[atomicAdd( &e.cursor[1], 1 )] = p;
  else e.plainJobs[atomicAdd( &e.cursor[2], 1 )] = p;
}

__global__ __launch_bounds__( 256 ) void mmvd_scatter_kernel( const int *__restrict__ slot, const unsigned long long *__restrict__ dist, int rows, unsigned long long *__restrict__ distOut )
{
  const int r = ( int ) ( blockIdx.x * blockDim.x + threadIdx.x );
  if( r < rows ) distOut[slot[r]] = dist[r];
}

template<int THREADS, int JPB>
int mmvd_fused_launch( vtmhip_ctx *ctx, const vtmhip_pic_params *pic, const int16_t *d_orgBase, const int16_t *d_refBase, const vtmhip_mmvd_job *d_jobs, int n,
                       int maxWidth, int maxHeight, int useSatd, vtmhip_mmvd_cand *d_cand, uint64_t *d_dist )
{
  // candidates per item: up to 8 share one load of the original block, fewer while the batch would leave the device short of workgroups (a lane group walks its
  // candidates one after the other, so a few CUs with 8 candidates per group are a handful of long latency chains)
  int cpi = 8;
  while( cpi > 1 && ( long ) n * ( VTMHIP_MMVD_NUM_CAND / cpi ) / JPB < 8L * ctx->numCUs ) cpi >>= 1;
  const size_t lds   = ( size_t ) JPB * mmvd_group_samples( maxWidth, maxHeight, THREADS <= 64 ) * sizeof( int16_t );
  const int    items = n * ( VTMHIP_MMVD_NUM_CAND / cpi );
  if( lds > 64 * 1024 )
    VTMHIP_HIP( ctx, hipFuncSetAttribute( reinterpret_cast<const void *>( mmvd_fused_kernel<THREADS, JPB> ), hipFuncAttributeMaxDynamicSharedMemorySize, ( int ) lds ) );
  hipLaunchKernelGGL( ( mmvd_fused_kernel<THREADS, JPB> ), dim3( ( items + JPB - 1 ) / JPB ), dim3( THREADS * JPB ), lds, ctx->stream, *pic, d_orgBase, d_refBase, d_jobs, items,
                      cpi, maxWidth, maxHeight, useSatd, d_cand, ( unsigned long long * ) d_dist );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

bool mmvd_pic_ok( const vtmhip_pic_params *pic )
{
  return pic && pic->picW > 0 && pic->picH > 0 && pic->ctuSize >= 16 && pic->ctuSize <= 128 && pic->bitDepth >= 8 && pic->bitDepth <= 12;
}

}   // namespace

extern "C"
{

int vtmhip_mmvd_struct_size( int which )
{
  switch( which )
  {
  case 0: return ( int ) sizeof( vtmhip_mmvd_job );
  case 1: return ( int ) sizeof( vtmhip_mmvd_cand );
  case 2: return ( int ) sizeof( vtmhip_mmvd_base );
  default: return -1;
  }
}

int vtmhip_mmvd_cands_host( const vtmhip_mmvd_job *job, const vtmhip_pic_params *pic, vtmhip_mmvd_cand out[64], int32_t predMv[64][2][2] )
{
  if( !job || !out || !predMv || !mmvd_pic_ok( pic ) || !mmvdJobOk( *job ) || job->bitDepth != pic->bitDepth ) return VTMHIP_E_INVALID;
  for( int c = 0; c < VTMHIP_MMVD_NUM_CAND; c++ )
  {
    int mode;
    mmvdDerive( *job, pic->picW, pic->picH, pic->ctuSize, c, out[c], mode, predMv[c] );
  }
  return VTMHIP_OK;
}

int vtmhip_mmvd_cand_satd_batch_dev( vtmhip_ctx *ctx, const vtmhip_pic_params *pic, const int16_t *d_orgBase, const int16_t *d_refBase, const vtmhip_mmvd_job *d_jobs,
                                     int n, int maxWidth, int maxHeight, int useSatd, vtmhip_mmvd_cand *d_cand, uint64_t *d_dist )
{
  VTMHIP_BATCH_ENTRY( ctx, n, d_orgBase && d_refBase && d_jobs && d_cand && d_dist );
  VTMHIP_REQUIRE( ctx, mmvd_pic_ok( pic ), "pic: sizes, ctuSize 16 .. 128, bitDepth 8 .. 12" );
  const int lanes = vtmhip_mc_lanes_per_block( maxWidth, maxHeight );
  VTMHIP_REQUIRE( ctx, lanes != 0 && mmvdSideOk( maxWidth ) && mmvdSideOk( maxHeight ), "maxWidth / maxHeight: powers of two in 4 .. 128" );
  // the route: the fused kernel up to a wave per block, the expansion for the workgroup-sized blocks (64 x 64 and up), where it measured faster;
  // VTMHIP_MMVD_FUSED = 0 / 1 sends every batch through the expansion / the fused kernel
  static const int fusedEnv = env_int( "VTMHIP_MMVD_FUSED", -1 );
  const bool       fused    = fusedEnv < 0 ? lanes != 256 : fusedEnv != 0;

  // the job table decides the expansion's row counts and is checked before anything runs
  HostStage              hs( ctx );
  const vtmhip_mmvd_job *jobs = nullptr;
  VTMHIP_TRY( hs.pull_table( d_jobs, n, jobs ) );
  size_t rows = 0, nBdof = 0, nPlain = 0, nWeighted = 0;
  for( int i = 0; i < n; i++ )
  {
    VTMHIP_REQUIRE( ctx, mmvdJobOk( jobs[i] ) && jobs[i].width <= maxWidth && jobs[i].height <= maxHeight && jobs[i].bitDepth == pic->bitDepth,
                    "mmvd job: sides 4..128 (powers of two, not 4x4, inside maxWidth x maxHeight), numBase 1..2, numSteps 1..8, a base without a list, bitDepth 8..12 and "
                    "pic's, strides >= width, BCW weight in {-2, 3, 4, 5, 10}" );
    if( fused ) { nBdof += ( size_t ) mmvdNumBdof( jobs[i] ); continue; }
    for( int c = 0; c < VTMHIP_MMVD_NUM_CAND; c++ )
    {
      vtmhip_mmvd_cand rec;
      int              mode;
      int32_t          pmv[2][2];
      mmvdDerive( jobs[i], pic->picW, pic->picH, pic->ctuSize, c, rec, mode, pmv );
      if( rec.kind == VTMHIP_MMVD_BDOF ) nBdof++;
      else if( rec.kind == VTMHIP_MMVD_PLAIN && mode == MMVD_PRED_BI && rec.bcwWeightL1 != MMVD_BCW_DEFAULT ) nWeighted++;
      else if( rec.kind == VTMHIP_MMVD_PLAIN ) nPlain++;
    }
  }
  rows = nBdof + nPlain + nWeighted;

  if( fused )
  {
    VTMHIP_TIME_KERNEL( ctx, "mmvd_fused_kernel" );
    if( lanes == 256 ) VTMHIP_TRY( ( mmvd_fused_launch<256, 1>( ctx, pic, d_orgBase, d_refBase, d_jobs, n, maxWidth, maxHeight, useSatd, d_cand, d_dist ) ) );
    else if( lanes == 64 ) VTMHIP_TRY( ( mmvd_fused_launch<64, 1>( ctx, pic, d_orgBase, d_refBase, d_jobs, n, maxWidth, maxHeight, useSatd, d_cand, d_dist ) ) );
    else if( lanes == 16 ) VTMHIP_TRY( ( mmvd_fused_launch<16, 4>( ctx, pic, d_orgBase, d_refBase, d_jobs, n, maxWidth, maxHeight, useSatd, d_cand, d_dist ) ) );
    else VTMHIP_TRY( ( mmvd_fused_launch<8, 8>( ctx, pic, d_orgBase, d_refBase, d_jobs, n, maxWidth, maxHeight, useSatd, d_cand, d_dist ) ) );
    if( rows == 0 ) return VTMHIP_OK;
  }

  const int    area = maxWidth * maxHeight;
  WorkPlan     wp;
  const size_t oCursor = wp.region<int>( 4 ), oSlot = wp.region<int>( rows ), oDist = wp.region<unsigned long long>( rows ), oDistJobs = wp.region<vtmhip_dist_job>( rows ),
               oBdof = wp.region<vtmhip_pred_job>( nBdof ), oPlain = wp.region<vtmhip_pred_job>( nPlain ), oMc = wp.region<vtmhip_mc_job>( 2 * nWeighted ),
               oPel = wp.region<vtmhip_pelop_job>( nWeighted ), oInter = wp.region<int16_t>( 2 * nWeighted * area ), oPred = wp.region<int16_t>( rows * area );
  VTMHIP_TRY( wp.reserve( ctx, VTMHIP_WORK_MMVD ) );
  MmvdExpand e;
  e.cursor = wp.at<int>( oCursor ); e.slot = wp.at<int>( oSlot ); e.dist = wp.at<unsigned long long>( oDist ); e.distJobs = wp.at<vtmhip_dist_job>( oDistJobs );
  e.bdofJobs = wp.at<vtmhip_pred_job>( oBdof ); e.plainJobs = wp.at<vtmhip_pred_job>( oPlain ); e.mcJobs = wp.at<vtmhip_mc_job>( oMc ); e.pelJobs = wp.at<vtmhip_pelop_job>( oPel );
  int16_t *d_inter = wp.at<int16_t>( oInter ), *d_pred = wp.at<int16_t>( oPred );
  VTMHIP_HIP( ctx, hipMemsetAsync( e.cursor, 0, 4 * sizeof( int ), ctx->stream ) );
  hipLaunchKernelGGL( mmvd_expand_kernel, dim3( ( n * VTMHIP_MMVD_NUM_CAND + 255 ) / 256 ), dim3( 256 ), 0, ctx->stream, *pic, d_jobs, n, area, useSatd, fused ? 0 : 1, e, d_cand,
                      ( unsigned long long * ) d_dist );
  VTMHIP_LAUNCHED( ctx );
  if( rows == 0 ) return VTMHIP_OK;
  if( nPlain ) VTMHIP_TRY( vtmhip_motion_compensation_batch_dev( ctx, nullptr, d_refBase, d_pred, nullptr, e.plainJobs, ( int ) nPlain, maxWidth, maxHeight ) );
  if( nWeighted )
  {
    VTMHIP_TRY( vtmhip_mc_batch_dev( ctx, d_refBase, d_inter, e.mcJobs, ( int ) ( 2 * nWeighted ), maxWidth, maxHeight ) );
    VTMHIP_TRY( vtmhip_add_weighted_avg_batch_dev( ctx, d_inter, d_inter, d_pred, e.pelJobs, ( int ) nWeighted ) );
  }
  if( nBdof ) VTMHIP_TRY( vtmhip_bdof_batch_dev( ctx, nullptr, d_refBase, d_pred, nullptr, e.bdofJobs, ( int ) nBdof, maxWidth, maxHeight ) );
  VTMHIP_TRY( vtmhip_dist_batch_dev( ctx, d_orgBase, d_pred, e.distJobs, ( int ) rows, ( uint64_t * ) e.dist ) );
  hipLaunchKernelGGL( mmvd_scatter_kernel, dim3( ( unsigned ) ( ( rows + 255 ) / 256 ) ), dim3( 256 ), 0, ctx->stream, e.slot, e.dist, ( int ) rows, ( unsigned long long * ) d_dist );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

}   // extern "C"
