// intra_chroma.hip -- intra chroma prediction for 4:2:0 on the device, Cb and Cr together; the rules are cclm_rules.hpp's and intra_rules.hpp's.
//   vtmhip_cclm_params                     IntraPrediction::xGetLMParameters, host arithmetic                          (CommonLib/IntraPrediction.cpp:1580-1795)
//   vtmhip_intra_chroma_pred_batch_dev     predIntraAng (chroma) / predIntraChromaLM for a batch of (block, mode) jobs  (:217-288)
//   vtmhip_intra_chroma_presel_batch_dev   the same predictions kept in LDS and reduced to SAD and SATD against the original Cb and Cr blocks: the pre-selection
//                                          of IntraSearch::estIntraPredChromaQT                                         (EncoderLib/IntraSearch.cpp:1308-1414)
//
// intra_chroma_shape_kernel: one workgroup walks the block table and leaves the lanes a job gets (vtmhip_intra_lanes_per_job of the largest well-formed block: 16
// up to 64 samples, 64 up to 1024) in the stream's workspace -- the tables stay on the device and the host never waits for them.
//
// intra_chroma_kernel<FUSED>: 256 threads.  A workgroup takes CHUNK consecutive jobs (16 / 8) and cuts them into runs of one block index.  Per run it stages in LDS
// the four lines (Cb / Cr x top / left), -- fused -- the two originals, and -- when the run holds an LM job -- the down-sampled luma ONCE: the inner W x H, the top
// row as far as MDLM_T reaches (W + min( aboveRight, H )) and the left column as far as MDLM_L reaches; every sample is cclmDsSample read straight from the luma
// plane (neighbouring lanes take neighbouring chroma positions, so a wave's six reads per sample fall in the same few cache lines).  Lanes 0 .. 5 then derive the
// six models (three LM modes x two components) from the staged template and lanes 254 / 255 the two DC values.  The run's jobs go through the lane groups: a group
// of L lanes forms both predictions of its job, 2 W H independent samples.
// Fused: a group writes its predictions to its slot of sPred and takes the four distortions from there through lanes_block_dist (dist_block.hpp).
// LDS: 4 lines x 72 + 1024 + 2 x 64 down-sampled samples + 6 models + 2 DC values = 3.1 KB; fused + 2 x 1024 (originals) + 4 x 2048 (slots): 23.1 KB.
// ich_chunk_body lives in intra_chroma_body.hpp: intra_chroma_chain.hip instantiates its third mode (predictions + residuals) in a kernel of its own.
#include "ctx.hpp"
#include "dist_block.hpp"
#include "cclm_rules.hpp"
#include "intra_chroma_body.hpp"   // ich_chunk_body, ich_lanes, ich_chunk, ich_block_ok: shared with intra_chroma_chain.hip

namespace
{

__global__ __launch_bounds__( 256 ) void intra_chroma_shape_kernel( const vtmhip_intra_chroma_block *__restrict__ blocks, int numBlocks, int *__restrict__ lanes )
{
  __shared__ int sMax;
  if( threadIdx.x == 0 ) sMax = 16;
  __syncthreads();
  int m = 0;
  for( int i = threadIdx.x; i < numBlocks; i += 256 )
  {
    const vtmhip_intra_chroma_block b = blocks[i];
    if( ich_block_ok( b ) ) m = max( m, b.width * b.height );
  }
  if( m ) atomicMax( &sMax, m );
  __syncthreads();
  if( threadIdx.x == 0 ) *lanes = ich_lanes( sMax );
}

template<bool FUSED>
__global__ __launch_bounds__( 256 ) void intra_chroma_kernel( const int *__restrict__ lanesPtr, const int16_t *__restrict__ refBase, const int16_t *__restrict__ lumaBase,
                                                              const int16_t *__restrict__ orgBase, const vtmhip_intra_chroma_block *__restrict__ blocks, int numBlocks,
                                                              const vtmhip_intra_chroma_job *__restrict__ jobs, int n, int16_t *__restrict__ predBase,
                                                              unsigned long long *__restrict__ dist )
{
  __shared__ int16_t   sLine[4 * ICH_LINE];
  __shared__ int16_t   sDs[ICH_MAX_AREA + 2 * ICH_EDGE];
  __shared__ CclmModel sModel[6];
  __shared__ int       sDc[2];
  __shared__ int16_t   sOrg[FUSED ? 2 * ICH_MAX_AREA : 1], sPred[FUSED ? 8 * ICH_MAX_AREA : 1];
  const int lanes = uni( *lanesPtr );
  if( ( long ) blockIdx.x * ich_chunk( lanes ) >= n ) return;
  const IchLds s = { sLine, sDs, sModel, sDc, sOrg, sPred };
  constexpr IchOut OUT = FUSED ? ICH_OUT_DIST : ICH_OUT_PRED;
  if( lanes == 16 ) ich_chunk_body<16, OUT>( s, refBase, lumaBase, orgBase, blocks, numBlocks, jobs, n, predBase, dist );
  else ich_chunk_body<64, OUT>( s, refBase, lumaBase, orgBase, blocks, numBlocks, jobs, n, predBase, dist );
}

int ich_launch( vtmhip_ctx *ctx, bool fused, const int16_t *d_refBase, const int16_t *d_lumaBase, const int16_t *d_orgBase, const vtmhip_intra_chroma_block *d_blocks,
                int numBlocks, const vtmhip_intra_chroma_job *d_jobs, int n, int16_t *d_predBase, uint64_t *d_dist )
{
  void *arena = nullptr;
  VTMHIP_TRY( vtmhip_internal_workspace( ctx, 256, &arena ) );
  int *d_lanes = ( int * ) arena;
  hipLaunchKernelGGL( intra_chroma_shape_kernel, dim3( 1 ), dim3( 256 ), 0, ctx->stream, d_blocks, numBlocks, d_lanes );
  VTMHIP_LAUNCHED( ctx );
  const dim3 grid( ( n + ICH_MIN_CHUNK - 1 ) / ICH_MIN_CHUNK );
  VTMHIP_TIME_KERNEL( ctx, fused ? "intra_chroma_presel_kernel" : "intra_chroma_pred_kernel" );
  if( fused )
    hipLaunchKernelGGL( intra_chroma_kernel<true>, grid, dim3( 256 ), 0, ctx->stream, d_lanes, d_refBase, d_lumaBase, d_orgBase, d_blocks, numBlocks, d_jobs, n,
                        d_predBase, ( unsigned long long * ) d_dist );
  else
    hipLaunchKernelGGL( intra_chroma_kernel<false>, grid, dim3( 256 ), 0, ctx->stream, d_lanes, d_refBase, d_lumaBase, d_orgBase, d_blocks, numBlocks, d_jobs, n,
                        d_predBase, ( unsigned long long * ) d_dist );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

}   // namespace

extern "C"
{

int vtmhip_intra_chroma_struct_size( int which )
{
  switch( which )
  {
  case 0: return ( int ) sizeof( vtmhip_intra_chroma_block );
  case 1: return ( int ) sizeof( vtmhip_intra_chroma_job );
  case 2: return ( int ) sizeof( vtmhip_cclm_model );
  default: return -1;
  }
}

int vtmhip_cclm_params( const vtmhip_intra_chroma_block *block, const int16_t *refBase, const int16_t *lumaBase, int component, int mode, vtmhip_cclm_model *out )
{
  if( !block || !refBase || !lumaBase || !out || component < 0 || component > 1 || mode < CCLM_LM || mode > CCLM_MDLM_T || !ich_block_ok( *block ) ) return VTMHIP_E_INVALID;
  const CclmAvail V    = ich_avail( *block );
  const CclmLuma  luma = { lumaBase + block->lumaOff, block->lumaStride };
  const int16_t  *top  = refBase + ( component ? block->crRefOff : block->cbRefOff );
  const CclmModel m    = cclmModel( block->width, block->height, mode, block->bitDepth, V, top, top + 2 * block->width + 1,
                                    [&]( int i, int j ) { return cclmDsSample( luma, V, i, j ); } );
  out->a = m.a; out->b = m.b; out->shift = m.shift;
  return VTMHIP_OK;
}

int vtmhip_intra_chroma_pred_batch_dev( vtmhip_ctx *ctx, const int16_t *d_refBase, const int16_t *d_lumaBase, const vtmhip_intra_chroma_block *d_blocks, int numBlocks,
                                        const vtmhip_intra_chroma_job *d_jobs, int n, int16_t *d_predBase )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, numBlocks >= 0, "numBlocks" );
  VTMHIP_BATCH_ARGS( ctx, n, d_refBase && d_lumaBase && d_blocks && d_jobs && d_predBase );
  VTMHIP_REQUIRE( ctx, numBlocks > 0, "jobs without blocks" );
  return ich_launch( ctx, false, d_refBase, d_lumaBase, nullptr, d_blocks, numBlocks, d_jobs, n, d_predBase, nullptr );
}

int vtmhip_intra_chroma_presel_batch_dev( vtmhip_ctx *ctx, const int16_t *d_refBase, const int16_t *d_lumaBase, const int16_t *d_orgBase,
                                          const vtmhip_intra_chroma_block *d_blocks, int numBlocks, const vtmhip_intra_chroma_job *d_jobs, int n, uint64_t *d_dist )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, numBlocks >= 0, "numBlocks" );
  VTMHIP_BATCH_ARGS( ctx, n, d_refBase && d_lumaBase && d_orgBase && d_blocks && d_jobs && d_dist );
  VTMHIP_REQUIRE( ctx, numBlocks > 0, "jobs without blocks" );
  return ich_launch( ctx, true, d_refBase, d_lumaBase, d_orgBase, d_blocks, numBlocks, d_jobs, n, nullptr, d_dist );
}

}   // extern "C"
