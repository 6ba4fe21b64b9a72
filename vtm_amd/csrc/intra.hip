// intra.hip -- intra luma prediction on the device; the rules are intra_rules.hpp's.
//   vtmhip_intra_pred_params       IntraPrediction::initPredIntraParams, host arithmetic                      (CommonLib/IntraPrediction.cpp:356-444)
//   vtmhip_intra_pred_batch_dev    IntraPrediction::predIntraAng for a batch of (block, mode) jobs            (:217-266)
//   vtmhip_intra_presel_batch_dev  the same prediction kept in LDS and reduced to its SAD and SATD against the original block: the first-round pre-selection
//                                  of IntraSearch::estIntraPredLumaQT                                         (EncoderLib/IntraSearch.cpp:549-700)
//
// Every sample of every mode is a closed form over the two reference lines (intra_rules.hpp), so a job is W x H independent samples.
//
// intra_shape_kernel (intra_lanes.hpp): one workgroup walks the block table and leaves the lanes a job gets (vtmhip_intra_lanes_per_job of the largest well-formed block) in the
// stream's workspace -- the tables stay on the device and the host never waits for them.
//
// intra_kernel<FUSED>: 256 threads.  A job gets L lanes: 16 (blocks up to 64 samples: 16 jobs run side by side, 4 in a wave), 64 (up to 1024: a wave per job) or
// 256 (the workgroup).  A workgroup takes CHUNK consecutive jobs (16 / 8 / 4) and cuts them into runs of one block index.  Per run it loads the block's two lines
// once, forms the [1 2 1]-filtered lines and the DC value in LDS and -- fused -- stages the original block; the run's jobs then go through the lane groups.  The
// grid is sized for the smallest CHUNK; workgroups past the table's end leave at once.
// Fused: a group writes its prediction to its slot of sPred and takes SAD and SATD from there through lanes_block_dist (dist_block.hpp: the xGetHADs tile rule);
// with 256 lanes per job wave 0 takes the SAD and wave 1 the SATD (64 x 64 is 64 tiles: one per lane).
// LDS: 4 lines x 136 samples + the DC value, fused + 2 x 4096 samples (original, predictions): 1.1 KB / 17.1 KB per workgroup.
// intra_chunk_body lives in intra_body.hpp: intra_chain.hip instantiates its third mode (prediction + residual) in a kernel of its own.
#include "ctx.hpp"
#include "chroma_taps.hpp"
#include "dist_block.hpp"
#include "intra_lanes.hpp"   // intra_lanes, intra_chunk, intra_shape_kernel: shared with mip.hip
#include "intra_rules.hpp"
#include "intra_body.hpp"    // intra_chunk_body: shared with intra_chain.hip

namespace
{

template<bool FUSED>
__global__ __launch_bounds__( 256 ) void intra_kernel( const int *__restrict__ lanesPtr, const int16_t *__restrict__ refBase, const int16_t *__restrict__ orgBase,
                                                       const vtmhip_intra_block *__restrict__ blocks, int numBlocks, const vtmhip_intra_job *__restrict__ jobs, int n,
                                                       int16_t *__restrict__ predBase, unsigned long long *__restrict__ dist )
{
  __shared__ int16_t sLine[4 * INTRA_LINE];
  __shared__ int     sDc;
  __shared__ int16_t sOrg[FUSED ? INTRA_MAX_AREA : 1], sPred[FUSED ? INTRA_MAX_AREA : 1];
  const int lanes = uni( *lanesPtr );
  if( ( long ) blockIdx.x * intra_chunk( lanes ) >= n ) return;
  const IntraLds s = { sLine, &sDc, sOrg, sPred };
  constexpr IntraOut OUT = FUSED ? INTRA_OUT_DIST : INTRA_OUT_PRED;
  if( lanes == 16 ) intra_chunk_body<16, OUT>( s, refBase, orgBase, blocks, numBlocks, jobs, n, predBase, dist );
  else if( lanes == 64 ) intra_chunk_body<64, OUT>( s, refBase, orgBase, blocks, numBlocks, jobs, n, predBase, dist );
  else intra_chunk_body<256, OUT>( s, refBase, orgBase, blocks, numBlocks, jobs, n, predBase, dist );
}

int intra_launch( vtmhip_ctx *ctx, bool fused, const int16_t *d_refBase, const int16_t *d_orgBase, const vtmhip_intra_block *d_blocks, int numBlocks,
                  const vtmhip_intra_job *d_jobs, int n, int16_t *d_predBase, uint64_t *d_dist )
{
  void *arena = nullptr;
  VTMHIP_TRY( vtmhip_internal_workspace( ctx, 256, &arena ) );
  int *d_lanes = ( int * ) arena;
  hipLaunchKernelGGL( intra_shape_kernel, dim3( 1 ), dim3( 256 ), 0, ctx->stream, d_blocks, numBlocks, d_lanes );
  VTMHIP_LAUNCHED( ctx );
  const dim3 grid( ( n + INTRA_MIN_CHUNK - 1 ) / INTRA_MIN_CHUNK );
  VTMHIP_TIME_KERNEL( ctx, fused ? "intra_presel_kernel" : "intra_pred_kernel" );
  if( fused )
    hipLaunchKernelGGL( intra_kernel<true>, grid, dim3( 256 ), 0, ctx->stream, d_lanes, d_refBase, d_orgBase, d_blocks, numBlocks, d_jobs, n, d_predBase,
                        ( unsigned long long * ) d_dist );
  else
    hipLaunchKernelGGL( intra_kernel<false>, grid, dim3( 256 ), 0, ctx->stream, d_lanes, d_refBase, d_orgBase, d_blocks, numBlocks, d_jobs, n, d_predBase,
                        ( unsigned long long * ) d_dist );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

}   // namespace

extern "C"
{

int vtmhip_intra_struct_size( int which )
{
  switch( which )
  {
  case 0: return ( int ) sizeof( vtmhip_intra_params );
  case 1: return ( int ) sizeof( vtmhip_intra_block );
  case 2: return ( int ) sizeof( vtmhip_intra_job );
  default: return -1;
  }
}

int vtmhip_intra_lanes_per_job( int maxArea ) { return intra_lanes( maxArea ); }

int vtmhip_intra_pred_params( int width, int height, int mode, int multiRefIdx, vtmhip_intra_params *out )
{
  if( !out || !intraBlockOk( width, height, 8, multiRefIdx ) || !intraModeOk( mode, multiRefIdx ) ) return VTMHIP_E_INVALID;
  intraPredParams( width, height, mode, multiRefIdx, *out );
  return VTMHIP_OK;
}

int vtmhip_intra_pred_batch_dev( vtmhip_ctx *ctx, const int16_t *d_refBase, const vtmhip_intra_block *d_blocks, int numBlocks, const vtmhip_intra_job *d_jobs, int n,
                                 int16_t *d_predBase )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, numBlocks >= 0, "numBlocks" );
  VTMHIP_BATCH_ARGS( ctx, n, d_refBase && d_blocks && d_jobs && d_predBase );
  VTMHIP_REQUIRE( ctx, numBlocks > 0, "jobs without blocks" );
  return intra_launch( ctx, false, d_refBase, nullptr, d_blocks, numBlocks, d_jobs, n, d_predBase, nullptr );
}

int vtmhip_intra_presel_batch_dev( vtmhip_ctx *ctx, const int16_t *d_refBase, const int16_t *d_orgBase, const vtmhip_intra_block *d_blocks, int numBlocks,
                                   const vtmhip_intra_job *d_jobs, int n, uint64_t *d_dist )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, numBlocks >= 0, "numBlocks" );
  VTMHIP_BATCH_ARGS( ctx, n, d_refBase && d_orgBase && d_blocks && d_jobs && d_dist );
  VTMHIP_REQUIRE( ctx, numBlocks > 0, "jobs without blocks" );
  return intra_launch( ctx, true, d_refBase, d_orgBase, d_blocks, numBlocks, d_jobs, n, nullptr, d_dist );
}

}   // extern "C"
