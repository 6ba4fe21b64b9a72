// intra_chroma_chain.hip -- one full-RD level of the intra chroma search on the device, Cb, Cr and joint Cb-Cr; the table rules are intra_chroma_chain_rules.hpp's.
//   vtmhip_intra_chroma_chain_batch_dev   per candidate the chroma branch of IntraSearch::xIntraCodingTUBlock under xRecurIntraChromaCodingQT: prediction, residual,
//                                         (scaling,) (forward ICT,) xT -> quant -> dequant -> xIT, (inverse ICT,) (inverse scaling,) clipped reconstruction and its
//                                         SSE against the original                                                 (EncoderLib/IntraSearch.cpp:3196-3318, 4934-5260)
//   vtmhip_intra_chroma_chain_make_jobs   the same checks and expansion as host arithmetic
//
// The launches of a call, all on the context's stream, nothing through the host between them:
//   intra_chroma_resi_kernel           the body of intra_chroma_body.hpp in its third mode: both predictions of every job and original - prediction (unscaled: the
//                                      chains scale on load)
//   intra_chroma_chain_expand_kernel   one thread per single job and per joint job: the vtmhip_tu_job / vtmhip_jccr_job of the chains (the residuals of the named
//                                      prediction at stride W, shape and bit depth of its block) and the block index, in the stream's workspace
//   the chains                         vtmhip_internal_tu_chain_launch / _crs_launch (transform.hip) and vtmhip_internal_jccr_chain_launch (jccr.hip), unchanged
//                                      kernels: levels and the reconstructed residuals at outOff.  The CRS instantiations run when some job carries an adj
//   intra_chroma_chain_finish_kernel<L>  one item per component block: nTu + 2 nJoint of them.  An item gets L lanes (16 up to 256 samples: sixteen items per
//                                      workgroup; 64 above: a wave per item), chosen by the host from the largest TU.  It decodes the item and runs
//                                      chain_finish.hpp's walk, as intra_chain_finish_kernel does: the reconstructed residual becomes
//                                      clip( prediction + residual ), and its SSE against the original joins the chains' results.  No LDS, no barrier.
// The entry reads the four tables back through HostStage (stage.hpp) and checks them (one stream synchronisation), so the kernels here trust what they are given.
// Its workspace is a WorkPlan in the slot VTMHIP_WORK_INTRA_CHROMA_CHAIN.
#include "ctx.hpp"
#include "stage.hpp"
#include "chain_finish.hpp"
#include "intra_chroma_body.hpp"   // ich_chunk_body, as intra_chroma.hip's kernels use it
#include "intra_chroma_chain_rules.hpp"

namespace
{

// The third mode of the prediction body (ICH_OUT_RESI): the two originals are staged in LDS as for the fused pre-selection, and a lane writes its sample to
// predBase and original - sample to resiBase, same offset, from the same register -- no Hadamard stage, no prediction slots in LDS (7.0 KB).  The entry has read
// the block table, so the lanes per job come by value and the grid is exact.
__global__ __launch_bounds__( 256 ) void intra_chroma_resi_kernel( int lanes, const int16_t *__restrict__ refBase, const int16_t *__restrict__ lumaBase,
                                                                   const int16_t *__restrict__ orgBase, const vtmhip_intra_chroma_block *__restrict__ blocks, int numBlocks,
                                                                   const vtmhip_intra_chroma_job *__restrict__ jobs, int n, int16_t *__restrict__ predBase,
                                                                   int16_t *__restrict__ resiBase )
{
  __shared__ int16_t   sLine[4 * ICH_LINE];
  __shared__ int16_t   sDs[ICH_MAX_AREA + 2 * ICH_EDGE];
  __shared__ CclmModel sModel[6];
  __shared__ int       sDc[2];
  __shared__ int16_t   sOrg[2 * ICH_MAX_AREA];
  const IchLds s = { sLine, sDs, sModel, sDc, sOrg, nullptr };
  if( lanes == 16 ) ich_chunk_body<16, ICH_OUT_RESI>( s, refBase, lumaBase, orgBase, blocks, numBlocks, jobs, n, predBase, nullptr, resiBase );
  else ich_chunk_body<64, ICH_OUT_RESI>( s, refBase, lumaBase, orgBase, blocks, numBlocks, jobs, n, predBase, nullptr, resiBase );
}

// threads 0 .. nTu - 1: the single jobs, nTu .. nTu + nJoint - 1: the joint jobs
__global__ __launch_bounds__( 256 ) void intra_chroma_chain_expand_kernel( const vtmhip_intra_chroma_block *__restrict__ blocks, const vtmhip_intra_chroma_job *__restrict__ jobs,
                                                                           const vtmhip_intra_chroma_tu_job *__restrict__ tuJobs, int nTu,
                                                                           const vtmhip_intra_chroma_joint_job *__restrict__ jointJobs, int nJoint,
                                                                           vtmhip_tu_job *__restrict__ outTu, int *__restrict__ tuBlock,
                                                                           vtmhip_jccr_job *__restrict__ outJoint, int *__restrict__ jointBlock )
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if( i < nTu )
  {
    const vtmhip_intra_chroma_tu_job t = tuJobs[i];
    const vtmhip_intra_chroma_job    p = jobs[t.pred];
    ichainExpandTu( t, blocks[p.block], p, outTu[i] );
    tuBlock[i] = p.block;
  }
  else if( i < nTu + nJoint )
  {
    const int k = i - nTu;
    const vtmhip_intra_chroma_joint_job t = jointJobs[k];
    const vtmhip_intra_chroma_job       p = jobs[t.pred];
    ichainExpandJoint( t, blocks[p.block], p, outJoint[k] );
    jointBlock[k] = p.block;
  }
}

struct IchFinishArgs
{
  const int16_t *orgBase, *predBase;
  const vtmhip_intra_chroma_block  *blocks;
  const vtmhip_intra_chroma_tu_job *tuJobs;      // the caller's table: the component of a single job
  const int                *tuBlock, *jointBlock;
  const vtmhip_tu_job      *xTu;
  const vtmhip_tu_result   *xTuRes;
  const vtmhip_jccr_job    *xJoint;
  const vtmhip_jccr_result *xJointRes;
  int                       nTu, nJoint;
  int16_t                  *recoBase, *recoCrBase;
  vtmhip_intra_tu_result           *results;
  vtmhip_intra_chroma_joint_result *jointResults;
};

// item i < nTu: single job i; item nTu + 2 k + c: component c of joint job k
template<int L>
__global__ __launch_bounds__( 256 ) void intra_chroma_chain_finish_kernel( const IchFinishArgs a )
{
  constexpr int G = 256 / L;
  const int g = threadIdx.x / L, l = threadIdx.x % L, i = blockIdx.x * G + g, n = a.nTu + 2 * a.nJoint;
  const int k = i < a.nTu ? i : ( i - a.nTu ) >> 1;   // the job
  int       c = 0;                                     // the component
  unsigned long long acc = 0;
  if( i < n )
  {
    int            w, h, bd;
    const int16_t *pred;
    int16_t       *reco;
    const vtmhip_intra_chroma_block *B;
    if( i < a.nTu )
    {
      const vtmhip_tu_job T = a.xTu[k];
      c = a.tuJobs[k].component;
      w = T.width; h = T.height; bd = T.bitDepth;
      pred = a.predBase + T.resiOff;   // the job's residual lies where its prediction does
      reco = a.recoBase + T.outOff;
      B    = a.blocks + a.tuBlock[k];
    }
    else
    {
      const vtmhip_jccr_job J = a.xJoint[k];
      c = ( i - a.nTu ) & 1;
      w = J.width; h = J.height; bd = J.bitDepth;
      pred = a.predBase + ( c ? J.crOff : J.cbOff );
      reco = ( c ? a.recoCrBase : a.recoBase ) + J.outOff;
      B    = a.blocks + a.jointBlock[k];
    }
    acc = chain_finish_walk<L>( pred, reco, a.orgBase + ( c ? B->crOrgOff : B->cbOrgOff ), B->orgStride, w, h, bd, l );
  }
  acc = chain_finish_group_sum<L>( acc );
  if( i < n && l == 0 )
  {
    if( i < a.nTu ) a.results[k] = chain_finish_result( acc, a.xTuRes[k] );
    else if( c == 0 )   // the Cb item also carries over what the joint chain left; the Cr item owns sseCr alone
    {
      const vtmhip_jccr_result t = a.xJointRes[k];
      vtmhip_intra_chroma_joint_result &r = a.jointResults[k];
      r.sseCb = acc; r.sseResiCb = t.sseCb; r.sseResiCr = t.sseCr; r.fwdDist = t.fwdDist; r.sumAbs = t.sumAbs; r.absSum = t.absSum;
    }
    else a.jointResults[k].sseCr = acc;
  }
}

}   // namespace

extern "C"
{

int vtmhip_intra_chroma_chain_struct_size( int which )
{
  switch( which )
  {
  case 0: return ( int ) sizeof( vtmhip_intra_chroma_tu_job );
  case 1: return ( int ) sizeof( vtmhip_intra_chroma_joint_job );
  case 2: return ( int ) sizeof( vtmhip_intra_chroma_joint_result );
  default: return -1;
  }
}

int vtmhip_intra_chroma_chain_make_jobs( const vtmhip_intra_chroma_block *blocks, int numBlocks, const vtmhip_intra_chroma_job *jobs, int nPred,
                                         const vtmhip_intra_chroma_tu_job *tuJobs, int nTu, const vtmhip_intra_chroma_joint_job *jointJobs, int nJoint,
                                         vtmhip_tu_job *outTu, vtmhip_jccr_job *outJoint, int *maxWidth, int *maxHeight, int *uniformTu, int *uniformJoint, int *crs )
{
  if( numBlocks < 0 || nPred < 0 || nTu < 0 || nJoint < 0 ) return VTMHIP_E_INVALID;
  if( ( numBlocks && !blocks ) || ( nPred && !jobs ) || ( nTu && ( !tuJobs || !outTu ) ) || ( nJoint && ( !jointJobs || !outJoint ) ) ) return VTMHIP_E_INVALID;
  IchainPlan plan;
  if( !ichainMakeJobs( blocks, numBlocks, jobs, nPred, tuJobs, nTu, jointJobs, nJoint, outTu, outJoint, plan ) ) return VTMHIP_E_INVALID;
  if( maxWidth ) { maxWidth[0] = plan.tu.maxWidth; maxWidth[1] = plan.joint.maxWidth; }
  if( maxHeight ) { maxHeight[0] = plan.tu.maxHeight; maxHeight[1] = plan.joint.maxHeight; }
  if( uniformTu ) *uniformTu = plan.tu.uniform;
  if( uniformJoint ) *uniformJoint = plan.joint.uniform;
  if( crs ) *crs = plan.crs;
  return VTMHIP_OK;
}

int vtmhip_intra_chroma_chain_batch_dev( vtmhip_ctx *ctx, const int16_t *d_refBase, const int16_t *d_lumaBase, const int16_t *d_orgBase,
                                         const vtmhip_intra_chroma_block *d_blocks, int numBlocks, const vtmhip_intra_chroma_job *d_jobs, int nPred,
                                         const vtmhip_intra_chroma_tu_job *d_tuJobs, int nTu, const vtmhip_intra_chroma_joint_job *d_jointJobs, int nJoint,
                                         int16_t *d_predBase, int16_t *d_resiBase, int32_t *d_levelsBase, int16_t *d_recoBase, int16_t *d_recoCrBase,
                                         vtmhip_intra_tu_result *d_results, vtmhip_intra_chroma_joint_result *d_jointResults )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, numBlocks >= 0 && nPred >= 0 && nTu >= 0 && nJoint >= 0, "negative count" );
  if( nPred + nTu + nJoint == 0 ) return VTMHIP_OK;
  VTMHIP_REQUIRE( ctx, d_refBase && d_orgBase && d_blocks && d_jobs && d_predBase && d_resiBase, "null pointer" );
  VTMHIP_REQUIRE( ctx, !nTu || ( d_tuJobs && d_recoBase && d_results ), "null pointer" );
  VTMHIP_REQUIRE( ctx, !nJoint || ( d_jointJobs && d_recoBase && d_recoCrBase && d_jointResults ), "null pointer" );

  // the tables decide the launches and the chain kernels trust their jobs: read back and checked before anything runs
  HostStage    hs( ctx );
  const size_t bBlk = ( size_t ) numBlocks * sizeof( vtmhip_intra_chroma_block ), bJob = ( size_t ) nPred * sizeof( vtmhip_intra_chroma_job ),
               bTu = ( size_t ) nTu * sizeof( vtmhip_intra_chroma_tu_job ), bJoint = ( size_t ) nJoint * sizeof( vtmhip_intra_chroma_joint_job );
  const size_t oBlk = hs.region( bBlk ), oJob = hs.region( bJob ), oTu = hs.region( bTu ), oJoint = hs.region( bJoint );
  VTMHIP_TRY( hs.reserve() );
  VTMHIP_TRY( hs.pull( oBlk, d_blocks, bBlk ) );
  VTMHIP_TRY( hs.pull( oJob, d_jobs, bJob ) );
  VTMHIP_TRY( hs.pull( oTu, d_tuJobs, bTu ) );
  VTMHIP_TRY( hs.pull( oJoint, d_jointJobs, bJoint ) );
  VTMHIP_TRY( hs.sync() );
  IchainPlan plan;
  VTMHIP_REQUIRE( ctx,
                  ichainScan( hs.host<vtmhip_intra_chroma_block>( oBlk ), numBlocks, hs.host<vtmhip_intra_chroma_job>( oJob ), nPred,
                              hs.host<vtmhip_intra_chroma_tu_job>( oTu ), nTu, hs.host<vtmhip_intra_chroma_joint_job>( oJoint ), nJoint, plan ),
                  "intra chroma chain tables: sides 4 / 8 / 16 / 32, bitDepth 8..12, flags 0 / 1, consistent availability, block index, mode 0..69, pred inside the table, "
                  "component 0 / 1, cbfMask 1..3, signFlag 0 / 1, DCT2 or TRSKIP, qpRem 0..5, qpPer >= 0, chromaAdj <= 32767, reserved fields 0" );
  VTMHIP_REQUIRE( ctx, !plan.anyLm || d_lumaBase, "null pointer: an LM job without the luma plane" );

  const int lanes = ich_lanes( plan.maxBlockArea ), chunk = ich_chunk( lanes );   // what intra_chroma_shape_kernel would leave: here the host knows it
  if( nPred )
  {
    VTMHIP_TIME_KERNEL( ctx, "intra_chroma_resi_kernel" );
    hipLaunchKernelGGL( intra_chroma_resi_kernel, dim3( ( nPred + chunk - 1 ) / chunk ), dim3( 256 ), 0, ctx->stream, lanes, d_refBase, d_lumaBase, d_orgBase, d_blocks, numBlocks,
                        d_jobs, nPred, d_predBase, d_resiBase );
    VTMHIP_LAUNCHED( ctx );
  }
  if( nTu + nJoint == 0 ) return VTMHIP_OK;

  // workspace: the block index per job, the expanded jobs, the chains' results -- the single jobs' and the joint jobs' side by side
  WorkPlan     wp;
  const size_t oTuBlk = wp.region<int>( nTu ), oJBlk = wp.region<int>( nJoint ), oXTu = wp.region<vtmhip_tu_job>( nTu ), oXJoint = wp.region<vtmhip_jccr_job>( nJoint ),
               oTuRes = wp.region<vtmhip_tu_result>( nTu ), oJRes = wp.region<vtmhip_jccr_result>( nJoint );
  VTMHIP_TRY( wp.reserve( ctx, VTMHIP_WORK_INTRA_CHROMA_CHAIN ) );
  int                *d_tuBlock    = wp.at<int>( oTuBlk );
  int                *d_jointBlock = wp.at<int>( oJBlk );
  vtmhip_tu_job      *d_xTu        = wp.at<vtmhip_tu_job>( oXTu );
  vtmhip_jccr_job    *d_xJoint     = wp.at<vtmhip_jccr_job>( oXJoint );
  vtmhip_tu_result   *d_xTuRes     = wp.at<vtmhip_tu_result>( oTuRes );
  vtmhip_jccr_result *d_xJointRes  = wp.at<vtmhip_jccr_result>( oJRes );
  {
    VTMHIP_TIME_KERNEL( ctx, "intra_chroma_chain_expand_kernel" );
    hipLaunchKernelGGL( intra_chroma_chain_expand_kernel, dim3( ( nTu + nJoint + 255 ) / 256 ), dim3( 256 ), 0, ctx->stream, d_blocks, d_jobs, d_tuJobs, nTu, d_jointJobs, nJoint,
                        d_xTu, d_tuBlock, d_xJoint, d_jointBlock );
    VTMHIP_LAUNCHED( ctx );
  }
  if( nTu )
  {
    if( plan.crs )
      VTMHIP_TRY( vtmhip_internal_tu_chain_crs_launch( ctx, d_resiBase, d_xTu, nTu, plan.tu.maxWidth, plan.tu.maxHeight, plan.tu.uniform, d_levelsBase, d_recoBase, d_xTuRes ) );
    else
      VTMHIP_TRY( vtmhip_internal_tu_chain_launch( ctx, d_resiBase, d_xTu, nTu, plan.tu.maxWidth, plan.tu.maxHeight, plan.tu.uniform, d_levelsBase, d_recoBase, d_xTuRes ) );
  }
  if( nJoint )
    VTMHIP_TRY( vtmhip_internal_jccr_chain_launch( ctx, plan.crs != 0, d_resiBase, d_xJoint, nJoint, plan.joint.maxWidth, plan.joint.maxHeight, plan.joint.uniform, d_levelsBase, d_recoBase,
                                                   d_recoCrBase, d_xJointRes ) );
  const IchFinishArgs a = { d_orgBase, d_predBase, d_blocks, d_tuJobs, d_tuBlock, d_jointBlock, d_xTu, d_xTuRes, d_xJoint, d_xJointRes, nTu, nJoint,
                            d_recoBase, d_recoCrBase, d_results, d_jointResults };
  return chain_finish_launch( ctx, "intra_chroma_chain_finish_kernel", intra_chroma_chain_finish_kernel<16>, intra_chroma_chain_finish_kernel<64>,
                              plan.tu.maxArea > plan.joint.maxArea ? plan.tu.maxArea : plan.joint.maxArea, nTu + 2 * nJoint, a );
}

}   // extern "C"
