// intra_chain.hip -- one full-RD level of the intra luma search on the device; the table rules are intra_chain_rules.hpp's.
//   vtmhip_intra_chain_batch_dev     per (mode, transform candidate) the steps of IntraSearch::xIntraCodingTUBlock: prediction, residual, xT -> quant -> dequant -> xIT,
//                                    clipped reconstruction and its SSE against the original                     (EncoderLib/IntraSearch.cpp:2989-3320)
//   vtmhip_intra_chain_make_tu_jobs  the same checks and expansion as host arithmetic
//   vtmhip_intra_chain_lfnst_batch_dev   the same level with a second candidate table, the lfnstIdx 1 / 2 candidates: expanded by lfnst_chain.hip's lfnst_expand_kernel
//                                    behind the plain jobs in the workspace, run by its lfnst_chain_kernel, finished by a second launch of intra_chain_finish_kernel
//   vtmhip_intra_chain_lfnst_make_jobs   its checks and both expansions as host arithmetic
//
// The launches of a call, all on the context's stream, nothing through the host between them:
//   intra_resi_kernel / mip_resi_kernel   the bodies of intra_body.hpp / mip_body.hpp in their third mode: every prediction and original - prediction
//   intra_chain_expand_kernel   one thread per TU job: the vtmhip_tu_job of the fused chain (the residual of the named prediction at stride W, shape and bit depth of
//                               its block) and the block index, both in the stream's workspace
//   the fused chain             vtmhip_internal_tu_chain_launch (transform.hip), unchanged: levels and the reconstructed residual at outOff
//   intra_chain_finish_kernel<L>  a TU job gets L lanes (16 up to 256 samples: sixteen jobs per workgroup; 64 above: a wave per job), chosen by the host from the largest
//                               TU.  It decodes the job and runs chain_finish.hpp's walk: the reconstructed residual becomes clip( prediction + residual ), and
//                               its SSE against the original joins the chain's result.  No LDS, no barrier.
// The entry reads the tables back through HostStage (stage.hpp) and checks them (one stream synchronisation), so the kernels here trust what they are given.  Its
// workspace is a WorkPlan in the slot VTMHIP_WORK_INTRA_CHAIN.
#include "ctx.hpp"
#include "stage.hpp"
#include "chain_finish.hpp"
#include "intra_body.hpp"   // intra_chunk_body, as intra.hip's kernels use it
#include "mip_body.hpp"     // mip_chunk_body, as mip.hip's
#include "intra_chain_rules.hpp"
#include "lfnst_rules.hpp"

namespace
{

// The third mode of the two prediction bodies (INTRA_OUT_RESI / MIP_OUT_RESI): the original is staged in LDS as for the fused pre-selection, and a lane writes its
// sample to predBase + predOff and original - sample to resiBase + predOff from the same register -- no Hadamard stage, no prediction slot in LDS (9.1 / 10.4 KB).
// The entry has read the block table, so the lanes per job come by value and the grid is exact.
__global__ __launch_bounds__( 256 ) void intra_resi_kernel( int lanes, const int16_t *__restrict__ refBase, const int16_t *__restrict__ orgBase,
                                                            const vtmhip_intra_block *__restrict__ blocks, int numBlocks, const vtmhip_intra_job *__restrict__ jobs, int n,
                                                            int16_t *__restrict__ predBase, int16_t *__restrict__ resiBase )
{
  __shared__ int16_t sLine[4 * INTRA_LINE];
  __shared__ int     sDc;
  __shared__ int16_t sOrg[INTRA_MAX_AREA];
  const IntraLds s = { sLine, &sDc, sOrg, nullptr };
  if( lanes == 16 ) intra_chunk_body<16, INTRA_OUT_RESI>( s, refBase, orgBase, blocks, numBlocks, jobs, n, predBase, nullptr, resiBase );
  else if( lanes == 64 ) intra_chunk_body<64, INTRA_OUT_RESI>( s, refBase, orgBase, blocks, numBlocks, jobs, n, predBase, nullptr, resiBase );
  else intra_chunk_body<256, INTRA_OUT_RESI>( s, refBase, orgBase, blocks, numBlocks, jobs, n, predBase, nullptr, resiBase );
}

__global__ __launch_bounds__( 256 ) void mip_resi_kernel( int lanes, const uint8_t *__restrict__ tab, const int16_t *__restrict__ refBase, const int16_t *__restrict__ orgBase,
                                                          const vtmhip_intra_block *__restrict__ blocks, int numBlocks, const vtmhip_mip_job *__restrict__ jobs, int n,
                                                          int16_t *__restrict__ predBase, int16_t *__restrict__ resiBase )
{
  __shared__ int16_t sLine[2 * MIP_LINE];
  __shared__ int     sBdry[8], sIn[2 * MIP_MAX_INPUT];
  __shared__ int16_t sRed[16 * MIP_MAX_REDUCED];
  __shared__ int16_t sOrg[INTRA_MAX_AREA];
  const MipLds s = { sLine, sBdry, sIn, sRed, sOrg, nullptr };
  if( lanes == 16 ) mip_chunk_body<16, MIP_OUT_RESI>( s, tab, refBase, orgBase, blocks, numBlocks, jobs, n, predBase, nullptr, resiBase );
  else if( lanes == 64 ) mip_chunk_body<64, MIP_OUT_RESI>( s, tab, refBase, orgBase, blocks, numBlocks, jobs, n, predBase, nullptr, resiBase );
  else mip_chunk_body<256, MIP_OUT_RESI>( s, tab, refBase, orgBase, blocks, numBlocks, jobs, n, predBase, nullptr, resiBase );
}

__global__ __launch_bounds__( 256 ) void intra_chain_expand_kernel( const vtmhip_intra_block *__restrict__ blocks, const vtmhip_intra_job *__restrict__ intraJobs, int nIntra,
                                                                    const vtmhip_mip_job *__restrict__ mipJobs, const vtmhip_intra_tu_job *__restrict__ tuJobs, int n,
                                                                    vtmhip_tu_job *__restrict__ out, int *__restrict__ tuBlock )
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if( i >= n ) return;
  const vtmhip_intra_tu_job t = tuJobs[i];
  int     blk;
  int64_t predOff;
  intraChainPred( intraJobs, nIntra, mipJobs, t.pred, blk, predOff );
  intraChainExpand( t, blocks[blk], predOff, out[i] );
  tuBlock[i] = blk;
}

template<int L>
__global__ __launch_bounds__( 256 ) void intra_chain_finish_kernel( const int16_t *__restrict__ orgBase, const int16_t *__restrict__ predBase,
                                                                    const vtmhip_intra_block *__restrict__ blocks, const int *__restrict__ tuBlock,
                                                                    const vtmhip_tu_job *__restrict__ xJobs, const vtmhip_tu_result *__restrict__ xRes, int n,
                                                                    int16_t *recoBase, vtmhip_intra_tu_result *__restrict__ results )
{
  constexpr int G = 256 / L;
  const int g = threadIdx.x / L, l = threadIdx.x % L, i = blockIdx.x * G + g;
  unsigned long long acc = 0;
  if( i < n )
  {
    const vtmhip_tu_job      T = xJobs[i];
    const vtmhip_intra_block B = blocks[tuBlock[i]];
    // the job's residual lies where its prediction does
    acc = chain_finish_walk<L>( predBase + T.resiOff, recoBase + T.outOff, orgBase + B.orgOff, B.orgStride, T.width, T.height, T.bitDepth, l );
  }
  acc = chain_finish_group_sum<L>( acc );
  if( i < n && l == 0 ) results[i] = chain_finish_result( acc, xRes[i] );
}

}   // namespace

extern "C"
{

int vtmhip_intra_chain_struct_size( int which )
{
  switch( which )
  {
  case 0: return ( int ) sizeof( vtmhip_intra_tu_job );
  case 1: return ( int ) sizeof( vtmhip_intra_tu_result );
  default: return -1;
  }
}

int vtmhip_intra_chain_make_tu_jobs( const vtmhip_intra_block *blocks, int numBlocks, const vtmhip_intra_job *intraJobs, int nIntra, const vtmhip_mip_job *mipJobs,
                                     int nMip, const vtmhip_intra_tu_job *tuJobs, int nTu, vtmhip_tu_job *out, int *maxWidth, int *maxHeight, int *uniform )
{
  if( numBlocks < 0 || nIntra < 0 || nMip < 0 || nTu < 0 ) return VTMHIP_E_INVALID;
  if( ( numBlocks && !blocks ) || ( nIntra && !intraJobs ) || ( nMip && !mipJobs ) || ( nTu && ( !tuJobs || !out ) ) ) return VTMHIP_E_INVALID;
  IntraChainPlan plan;
  if( !intraChainMakeTuJobs( blocks, numBlocks, intraJobs, nIntra, mipJobs, nMip, tuJobs, nTu, out, plan ) ) return VTMHIP_E_INVALID;
  if( maxWidth ) *maxWidth = plan.tu.maxWidth;
  if( maxHeight ) *maxHeight = plan.tu.maxHeight;
  if( uniform ) *uniform = plan.tu.uniform;
  return VTMHIP_OK;
}

}   // extern "C"

// both level entries: vtmhip_intra_chain_batch_dev is nLfnst == 0
static int intra_chain_level( vtmhip_ctx *ctx, const int16_t *d_refBase, const int16_t *d_orgBase, const vtmhip_intra_block *d_blocks, int numBlocks,
                              const vtmhip_intra_job *d_intraJobs, int nIntra, const vtmhip_mip_job *d_mipJobs, int nMip, const vtmhip_intra_tu_job *d_tuJobs, int nTu,
                              const vtmhip_intra_lfnst_tu_job *d_lfnstJobs, int nLfnst, int16_t *d_predBase, int16_t *d_resiBase, int32_t *d_levelsBase, int16_t *d_recoBase,
                              vtmhip_intra_tu_result *d_results, vtmhip_intra_tu_result *d_lfnstResults )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, numBlocks >= 0 && nIntra >= 0 && nMip >= 0 && nTu >= 0 && nLfnst >= 0, "negative count" );
  if( nIntra + nMip + nTu + nLfnst == 0 ) return VTMHIP_OK;
  VTMHIP_REQUIRE( ctx, d_refBase && d_orgBase && d_blocks && d_predBase && d_resiBase && ( !nIntra || d_intraJobs ) && ( !nMip || d_mipJobs ), "null pointer" );
  VTMHIP_REQUIRE( ctx, !nTu || ( d_tuJobs && d_recoBase && d_results ), "null pointer" );
  VTMHIP_REQUIRE( ctx, !nLfnst || ( d_lfnstJobs && d_recoBase && d_lfnstResults ), "null pointer" );
  VTMHIP_REQUIRE( ctx, !nMip || ctx->mipTab, "vtmhip_mip_set_tables has not been called" );
  VTMHIP_REQUIRE( ctx, !nLfnst || ctx->lfnstTab, "vtmhip_lfnst_set_tables has not been called" );

  // the tables decide the launches and the chain kernels trust their jobs: read back and checked before anything runs
  HostStage    hs( ctx );
  const size_t bBlk = ( size_t ) numBlocks * sizeof( vtmhip_intra_block ), bIntra = ( size_t ) nIntra * sizeof( vtmhip_intra_job ),
               bMip = ( size_t ) nMip * sizeof( vtmhip_mip_job ), bTu = ( size_t ) nTu * sizeof( vtmhip_intra_tu_job ),
               bLf = ( size_t ) nLfnst * sizeof( vtmhip_intra_lfnst_tu_job );
  const size_t oBlk = hs.region( bBlk ), oIntra = hs.region( bIntra ), oMip = hs.region( bMip ), oTu = hs.region( bTu ), oLf = hs.region( bLf );
  VTMHIP_TRY( hs.reserve() );
  VTMHIP_TRY( hs.pull( oBlk, d_blocks, bBlk ) );
  VTMHIP_TRY( hs.pull( oIntra, d_intraJobs, bIntra ) );
  VTMHIP_TRY( hs.pull( oMip, d_mipJobs, bMip ) );
  VTMHIP_TRY( hs.pull( oTu, d_tuJobs, bTu ) );
  VTMHIP_TRY( hs.pull( oLf, d_lfnstJobs, bLf ) );
  VTMHIP_TRY( hs.sync() );
  const vtmhip_intra_block *blocks    = hs.host<vtmhip_intra_block>( oBlk );
  const vtmhip_intra_job   *intraJobs = hs.host<vtmhip_intra_job>( oIntra );
  const vtmhip_mip_job     *mipJobs   = hs.host<vtmhip_mip_job>( oMip );
  IntraChainPlan plan;
  VTMHIP_REQUIRE( ctx,
                  intraChainScan( blocks, numBlocks, intraJobs, nIntra, mipJobs, nMip, hs.host<vtmhip_intra_tu_job>( oTu ), nTu, plan ),
                  "intra chain tables: sides 4..64, bitDepth 8..12, multiRefIdx 0..2 (MIP: 0), block index, mode, pred inside the tables, qpRem 0..5, qpPer >= 0, "
                  "two of DCT2 / DCT8 / DST7 (DCT2 above 32) or both TRSKIP (sides up to 32), reserved fields 0" );
  LfnstPlan lplan;
  VTMHIP_REQUIRE( ctx,
                  lfnstLevelScan( blocks, intraJobs, nIntra, mipJobs, nMip, hs.host<vtmhip_intra_lfnst_tu_job>( oLf ), nLfnst, lplan ),
                  "intra chain LFNST table: lfnstIdx 1..2, pred inside the tables, MIP on sides >= 16 only, qpRem 0..5, qpPer >= 0, reserved fields 0" );

  const int lanes = intra_lanes( plan.maxBlockArea ), chunk = intra_chunk( lanes );   // what intra_shape_kernel would leave: here the host knows it
  if( nIntra )
  {
    VTMHIP_TIME_KERNEL( ctx, "intra_resi_kernel" );
    hipLaunchKernelGGL( intra_resi_kernel, dim3( ( nIntra + chunk - 1 ) / chunk ), dim3( 256 ), 0, ctx->stream, lanes, d_refBase, d_orgBase, d_blocks, numBlocks, d_intraJobs,
                        nIntra, d_predBase, d_resiBase );
    VTMHIP_LAUNCHED( ctx );
  }
  if( nMip )
  {
    VTMHIP_TIME_KERNEL( ctx, "mip_resi_kernel" );
    hipLaunchKernelGGL( mip_resi_kernel, dim3( ( nMip + chunk - 1 ) / chunk ), dim3( 256 ), 0, ctx->stream, lanes, ctx->mipTab, d_refBase, d_orgBase, d_blocks, numBlocks,
                        d_mipJobs, nMip, d_predBase, d_resiBase );
    VTMHIP_LAUNCHED( ctx );
  }
  if( nTu + nLfnst == 0 ) return VTMHIP_OK;

  // workspace: the block index per TU job, the expanded jobs, their results
  // the LFNST jobs follow the plain ones in all three arrays (their vtmhip_tu_job is the mirror the finish kernel reads); the LFNST chain's own jobs come last
  const size_t nAll = ( size_t ) nTu + nLfnst;
  WorkPlan     wp;
  const size_t oBlock = wp.region<int>( nAll ), oJobs = wp.region<vtmhip_tu_job>( nAll ), oRes = wp.region<vtmhip_tu_result>( nAll ),
               oChain = wp.region<vtmhip_lfnst_chain_job>( nLfnst );
  VTMHIP_TRY( wp.reserve( ctx, VTMHIP_WORK_INTRA_CHAIN ) );
  int                    *d_tuBlock = wp.at<int>( oBlock );
  vtmhip_tu_job          *d_xJobs   = wp.at<vtmhip_tu_job>( oJobs );
  vtmhip_tu_result       *d_xRes    = wp.at<vtmhip_tu_result>( oRes );
  vtmhip_lfnst_chain_job *d_cJobs   = wp.at<vtmhip_lfnst_chain_job>( oChain );
  if( nTu )
  {
    VTMHIP_TIME_KERNEL( ctx, "intra_chain_expand_kernel" );
    hipLaunchKernelGGL( intra_chain_expand_kernel, dim3( ( nTu + 255 ) / 256 ), dim3( 256 ), 0, ctx->stream, d_blocks, d_intraJobs, nIntra, d_mipJobs, d_tuJobs, nTu, d_xJobs,
                        d_tuBlock );
    VTMHIP_LAUNCHED( ctx );
  }
  if( nTu ) VTMHIP_TRY( vtmhip_internal_tu_chain_launch( ctx, d_resiBase, d_xJobs, nTu, plan.tu.maxWidth, plan.tu.maxHeight, plan.tu.uniform, d_levelsBase, d_recoBase, d_xRes ) );
  if( nLfnst )
  {
    VTMHIP_TRY( vtmhip_internal_lfnst_expand_launch( ctx, d_blocks, d_intraJobs, nIntra, d_mipJobs, d_lfnstJobs, nLfnst, d_cJobs, d_xJobs + nTu, d_tuBlock + nTu ) );
    VTMHIP_TRY( vtmhip_internal_lfnst_chain_launch( ctx, d_resiBase, d_cJobs, nLfnst, lplan.maxArea, lplan.jobInts, d_levelsBase, d_recoBase, d_xRes + nTu ) );
  }
  if( nTu )
    VTMHIP_TRY( chain_finish_launch( ctx, "intra_chain_finish_kernel", intra_chain_finish_kernel<16>, intra_chain_finish_kernel<64>, plan.tu.maxArea, nTu, d_orgBase, d_predBase,
                                     d_blocks, d_tuBlock, d_xJobs, d_xRes, nTu, d_recoBase, d_results ) );
  if( nLfnst )   // the same finish kernel over the second result table
    VTMHIP_TRY( chain_finish_launch( ctx, "intra_chain_finish_kernel", intra_chain_finish_kernel<16>, intra_chain_finish_kernel<64>, lplan.maxArea, nLfnst, d_orgBase, d_predBase,
                                     d_blocks, d_tuBlock + nTu, d_xJobs + nTu, d_xRes + nTu, nLfnst, d_recoBase, d_lfnstResults ) );
  return VTMHIP_OK;
}

extern "C"
{

int vtmhip_intra_chain_batch_dev( vtmhip_ctx *ctx, const int16_t *d_refBase, const int16_t *d_orgBase, const vtmhip_intra_block *d_blocks, int numBlocks,
                                  const vtmhip_intra_job *d_intraJobs, int nIntra, const vtmhip_mip_job *d_mipJobs, int nMip, const vtmhip_intra_tu_job *d_tuJobs,
                                  int nTu, int16_t *d_predBase, int16_t *d_resiBase, int32_t *d_levelsBase, int16_t *d_recoBase, vtmhip_intra_tu_result *d_results )
{
  return intra_chain_level( ctx, d_refBase, d_orgBase, d_blocks, numBlocks, d_intraJobs, nIntra, d_mipJobs, nMip, d_tuJobs, nTu, nullptr, 0, d_predBase, d_resiBase, d_levelsBase,
                            d_recoBase, d_results, nullptr );
}

int vtmhip_intra_chain_lfnst_batch_dev( vtmhip_ctx *ctx, const int16_t *d_refBase, const int16_t *d_orgBase, const vtmhip_intra_block *d_blocks, int numBlocks,
                                        const vtmhip_intra_job *d_intraJobs, int nIntra, const vtmhip_mip_job *d_mipJobs, int nMip, const vtmhip_intra_tu_job *d_tuJobs,
                                        int nTu, const vtmhip_intra_lfnst_tu_job *d_lfnstJobs, int nLfnst, int16_t *d_predBase, int16_t *d_resiBase,
                                        int32_t *d_levelsBase, int16_t *d_recoBase, vtmhip_intra_tu_result *d_results, vtmhip_intra_tu_result *d_lfnstResults )
{
  return intra_chain_level( ctx, d_refBase, d_orgBase, d_blocks, numBlocks, d_intraJobs, nIntra, d_mipJobs, nMip, d_tuJobs, nTu, d_lfnstJobs, nLfnst, d_predBase, d_resiBase,
                            d_levelsBase, d_recoBase, d_results, d_lfnstResults );
}

int vtmhip_intra_chain_lfnst_make_jobs( const vtmhip_intra_block *blocks, int numBlocks, const vtmhip_intra_job *intraJobs, int nIntra, const vtmhip_mip_job *mipJobs,
                                        int nMip, const vtmhip_intra_tu_job *tuJobs, int nTu, const vtmhip_intra_lfnst_tu_job *lfnstJobs, int nLfnst, vtmhip_tu_job *outTu,
                                        vtmhip_lfnst_chain_job *outLfnst, int *maxWidth, int *maxHeight, int *uniform, int *lanesOut )
{
  if( numBlocks < 0 || nIntra < 0 || nMip < 0 || nTu < 0 || nLfnst < 0 ) return VTMHIP_E_INVALID;
  if( ( numBlocks && !blocks ) || ( nIntra && !intraJobs ) || ( nMip && !mipJobs ) || ( nTu && ( !tuJobs || !outTu ) ) || ( nLfnst && ( !lfnstJobs || !outLfnst ) ) )
    return VTMHIP_E_INVALID;
  IntraChainPlan plan;
  LfnstPlan      lplan;
  if( !lfnstLevelMakeJobs( blocks, numBlocks, intraJobs, nIntra, mipJobs, nMip, tuJobs, nTu, lfnstJobs, nLfnst, outTu, outLfnst, plan, lplan ) ) return VTMHIP_E_INVALID;
  if( maxWidth ) *maxWidth = plan.tu.maxWidth;
  if( maxHeight ) *maxHeight = plan.tu.maxHeight;
  if( uniform ) *uniform = plan.tu.uniform;
  if( lanesOut ) *lanesOut = nLfnst ? lfnstLanes( lplan.maxArea ) : 0;
  return VTMHIP_OK;
}

}   // extern "C"
