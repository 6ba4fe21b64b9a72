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
//                                      workgroup; 64 above: a wave per item), chosen by the host from the largest TU.  A lane walks 4-sample row segments as
//                                      intra_chain_finish_kernel does: prediction and reconstructed residual are W x H contiguous, the original has its own stride;
//                                      all three come as one 8-byte access at a 2-byte aligned address (pel_pack.hpp).  It overwrites the reconstructed residual
//                                      with clip( prediction + residual ) and sums ( original - reconstruction )^2 with the per-addend 32-bit product of
//                                      dist_block.hpp's SSE; the group's lanes are added by shuffles.  No LDS, no barrier.
// The entry reads the four tables back and checks them (one stream synchronisation), so the kernels here trust what they are given.
#include "ctx.hpp"
#include "intra_chroma_body.hpp"   // ich_chunk_body, as intra_chroma.hip's kernels use it
#include "intra_chroma_chain_rules.hpp"
#include "pel_pack.hpp"

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
    const int      lgSegs = intraLog2( w ) - 2, items = ( w * h ) >> 2, maxVal = ( 1 << bd ) - 1, orgStride = B->orgStride;
    const int16_t *org = a.orgBase + ( c ? B->crOrgOff : B->cbOrgOff );
    for( int it = l; it < items; it += L )
    {
      const int y = it >> lgSegs, x = ( it & ( ( 1 << lgSegs ) - 1 ) ) << 2;
      int p[4], r[4], o[4];
      ld4( pred + 4 * it, 4, p );
      ld4( reco + 4 * it, 4, r );
      ld4( org + ( long ) y * orgStride + x, 4, o );
#pragma unroll
      for( int q = 0; q < 4; q++ )
      {
        r[q] = min( max( p[q] + r[q], 0 ), maxVal );
        const int d = o[q] - r[q];
        acc += ( unsigned long long ) ( ( unsigned ) d * ( unsigned ) d );
      }
      st4( reco + 4 * it, 4, r );
    }
  }
#pragma unroll
  for( int o = L >> 1; o > 0; o >>= 1 ) acc += __shfl_xor( acc, o, 64 );   // a group is L consecutive lanes of one wave, all of them here
  if( i < n && l == 0 )
  {
    if( i < a.nTu )
    {
      const vtmhip_tu_result t = a.xTuRes[k];
      vtmhip_intra_tu_result r;
      r.sse = acc; r.sseResi = t.sse; r.sumAbs = t.sumAbs; r.absSum = t.absSum;
      a.results[k] = r;
    }
    else if( c == 0 )   // the Cb item also carries over what the joint chain left; the Cr item owns sseCr alone
    {
      const vtmhip_jccr_result t = a.xJointRes[k];
      vtmhip_intra_chroma_joint_result &r = a.jointResults[k];
      r.sseCb = acc; r.sseResiCb = t.sseCb; r.sseResiCr = t.sseCr; r.fwdDist = t.fwdDist; r.sumAbs = t.sumAbs; r.absSum = t.absSum;
    }
    else a.jointResults[k].sseCr = acc;
  }
}

size_t align256( size_t v ) { return ( v + 255 ) & ~( size_t ) 255; }

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
  if( maxWidth ) { maxWidth[0] = plan.maxWidth[0]; maxWidth[1] = plan.maxWidth[1]; }
  if( maxHeight ) { maxHeight[0] = plan.maxHeight[0]; maxHeight[1] = plan.maxHeight[1]; }
  if( uniformTu ) *uniformTu = plan.uniform[0];
  if( uniformJoint ) *uniformJoint = plan.uniform[1];
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
  const size_t bBlk = ( size_t ) numBlocks * sizeof( vtmhip_intra_chroma_block ), bJob = ( size_t ) nPred * sizeof( vtmhip_intra_chroma_job ),
               bTu = ( size_t ) nTu * sizeof( vtmhip_intra_chroma_tu_job ), bJoint = ( size_t ) nJoint * sizeof( vtmhip_intra_chroma_joint_job );   // every record size is a multiple of 8
  VTMHIP_TRY( vtmhip_internal_scratch( ctx, bBlk + bJob + bTu + bJoint ) );
  char *host = ( char * ) ctx->pinned;
  if( bBlk ) VTMHIP_HIP( ctx, hipMemcpyAsync( host, d_blocks, bBlk, hipMemcpyDeviceToHost, ctx->stream ) );
  if( bJob ) VTMHIP_HIP( ctx, hipMemcpyAsync( host + bBlk, d_jobs, bJob, hipMemcpyDeviceToHost, ctx->stream ) );
  if( bTu ) VTMHIP_HIP( ctx, hipMemcpyAsync( host + bBlk + bJob, d_tuJobs, bTu, hipMemcpyDeviceToHost, ctx->stream ) );
  if( bJoint ) VTMHIP_HIP( ctx, hipMemcpyAsync( host + bBlk + bJob + bTu, d_jointJobs, bJoint, hipMemcpyDeviceToHost, ctx->stream ) );
  VTMHIP_HIP( ctx, hipStreamSynchronize( ctx->stream ) );
  IchainPlan plan;
  VTMHIP_REQUIRE( ctx,
                  ichainScan( ( const vtmhip_intra_chroma_block * ) host, numBlocks, ( const vtmhip_intra_chroma_job * ) ( host + bBlk ), nPred,
                              ( const vtmhip_intra_chroma_tu_job * ) ( host + bBlk + bJob ), nTu, ( const vtmhip_intra_chroma_joint_job * ) ( host + bBlk + bJob + bTu ),
                              nJoint, plan ),
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

  // workspace (slot 6; ctx.hpp lists the slots): the block index per job, the expanded jobs, the chains' results -- the single jobs' and the joint jobs' side by side
  const size_t oJBlk = align256( ( size_t ) nTu * sizeof( int ) ), oXTu = align256( oJBlk + ( size_t ) nJoint * sizeof( int ) ),
               oXJoint = align256( oXTu + ( size_t ) nTu * sizeof( vtmhip_tu_job ) ), oTuRes = align256( oXJoint + ( size_t ) nJoint * sizeof( vtmhip_jccr_job ) ),
               oJRes = align256( oTuRes + ( size_t ) nTu * sizeof( vtmhip_tu_result ) );
  void *arena = nullptr;
  VTMHIP_TRY( vtmhip_internal_workspace( ctx, oJRes + ( size_t ) nJoint * sizeof( vtmhip_jccr_result ), &arena, 6 ) );
  char *base = ( char * ) arena;
  int                *d_tuBlock    = ( int * ) base;
  int                *d_jointBlock = ( int * ) ( base + oJBlk );
  vtmhip_tu_job      *d_xTu        = ( vtmhip_tu_job * ) ( base + oXTu );
  vtmhip_jccr_job    *d_xJoint     = ( vtmhip_jccr_job * ) ( base + oXJoint );
  vtmhip_tu_result   *d_xTuRes     = ( vtmhip_tu_result * ) ( base + oTuRes );
  vtmhip_jccr_result *d_xJointRes  = ( vtmhip_jccr_result * ) ( base + oJRes );
  {
    VTMHIP_TIME_KERNEL( ctx, "intra_chroma_chain_expand_kernel" );
    hipLaunchKernelGGL( intra_chroma_chain_expand_kernel, dim3( ( nTu + nJoint + 255 ) / 256 ), dim3( 256 ), 0, ctx->stream, d_blocks, d_jobs, d_tuJobs, nTu, d_jointJobs, nJoint,
                        d_xTu, d_tuBlock, d_xJoint, d_jointBlock );
    VTMHIP_LAUNCHED( ctx );
  }
  if( nTu )
  {
    if( plan.crs )
      VTMHIP_TRY( vtmhip_internal_tu_chain_crs_launch( ctx, d_resiBase, d_xTu, nTu, plan.maxWidth[0], plan.maxHeight[0], plan.uniform[0], d_levelsBase, d_recoBase, d_xTuRes ) );
    else
      VTMHIP_TRY( vtmhip_internal_tu_chain_launch( ctx, d_resiBase, d_xTu, nTu, plan.maxWidth[0], plan.maxHeight[0], plan.uniform[0], d_levelsBase, d_recoBase, d_xTuRes ) );
  }
  if( nJoint )
    VTMHIP_TRY( vtmhip_internal_jccr_chain_launch( ctx, plan.crs != 0, d_resiBase, d_xJoint, nJoint, plan.maxWidth[1], plan.maxHeight[1], plan.uniform[1], d_levelsBase, d_recoBase,
                                                   d_recoCrBase, d_xJointRes ) );
  {
    const IchFinishArgs a = { d_orgBase, d_predBase, d_blocks, d_tuJobs, d_tuBlock, d_jointBlock, d_xTu, d_xTuRes, d_xJoint, d_xJointRes, nTu, nJoint,
                              d_recoBase, d_recoCrBase, d_results, d_jointResults };
    const int items = nTu + 2 * nJoint;
    VTMHIP_TIME_KERNEL( ctx, "intra_chroma_chain_finish_kernel" );
    if( ( plan.maxArea[0] > plan.maxArea[1] ? plan.maxArea[0] : plan.maxArea[1] ) <= 256 )
      hipLaunchKernelGGL( intra_chroma_chain_finish_kernel<16>, dim3( ( items + 15 ) / 16 ), dim3( 256 ), 0, ctx->stream, a );
    else
      hipLaunchKernelGGL( intra_chroma_chain_finish_kernel<64>, dim3( ( items + 3 ) / 4 ), dim3( 256 ), 0, ctx->stream, a );
    VTMHIP_LAUNCHED( ctx );
  }
  return VTMHIP_OK;
}

}   // extern "C"
