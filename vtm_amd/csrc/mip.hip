// mip.hip -- matrix-based intra prediction (MIP) of luma blocks on the device; the rules are mip_rules.hpp's.
//   vtmhip_mip_set_tables         the caller's trained matrices mipMatrix4x4 / 8x8 / 16x16 (CommonLib/MipData.h), copied to the context's device
//   vtmhip_mip_pred_host          MatrixIntraPrediction::prepareInputForPred + predBlock on the host, no context   (CommonLib/MatrixIntraPrediction.cpp:62-137)
//   vtmhip_mip_pred_batch_dev     the same for a batch of (block, mode, transposed) jobs
//   vtmhip_mip_presel_batch_dev   the same prediction kept in LDS and reduced to its SAD and SATD against the original block: the MIP candidates of
//                                 IntraSearch::estIntraPredLumaQT                                                  (EncoderLib/IntraSearch.cpp:749-793)
//
// mip_kernel<FUSED>: 256 threads, on the plan of intra_kernel (intra.hip).  A job gets L lanes -- 16, 64 or 256 by the largest well-formed block of the table
// (intra_lanes.hpp: the same one-workgroup kernel, so nothing is read back) -- and a workgroup takes CHUNK consecutive jobs (16 / 8 / 4), cut into runs of one block
// index.  Per run it loads top[1 .. W] and left[1 .. H] (nothing else of the lines is touched), -- fused -- stages the original block, and forms in LDS the two
// reduced boundaries, from them the two rebased inputs (top | left and left | top, 2 x 8 ints) and their input offsets, once for all the block's jobs.  Per job one
// lane per reduced sample multiplies its matrix row (4 / 8 / 7 bytes, read as bytes from the 4.6 KB table) with the input and writes the clipped value to the job's
// reduced block in LDS, transposed where asked; then all lanes of the job form the W x H samples from the closed form of mipSample.
// Fused: a group writes its prediction to its slot of sPred and takes SAD and SATD from there through lanes_block_dist (dist_block.hpp: the xGetHADs tile rule);
// with 256 lanes per job wave 0 takes the SAD and wave 1 the SATD.
// LDS: 2 lines x 72 samples + 8 + 16 ints + 16 reduced blocks x 64 samples, fused + 2 x 4096 samples (original, predictions): 2.4 KB / 18.4 KB per workgroup.
// mip_chunk_body lives in mip_body.hpp: intra_chain.hip instantiates its third mode (prediction + residual) in a kernel of its own.
#include "ctx.hpp"
#include "dist_block.hpp"
#include "intra_lanes.hpp"
#include "mip_rules.hpp"
#include "mip_body.hpp"   // mip_chunk_body: shared with intra_chain.hip

namespace
{

template<bool FUSED>
__global__ __launch_bounds__( 256 ) void mip_kernel( const int *__restrict__ lanesPtr, const uint8_t *__restrict__ tab, const int16_t *__restrict__ refBase,
                                                     const int16_t *__restrict__ orgBase, const vtmhip_intra_block *__restrict__ blocks, int numBlocks,
                                                     const vtmhip_mip_job *__restrict__ jobs, int n, int16_t *__restrict__ predBase, unsigned long long *__restrict__ dist )
{
  __shared__ int16_t sLine[2 * MIP_LINE];
  __shared__ int     sBdry[8], sIn[2 * MIP_MAX_INPUT];
  __shared__ int16_t sRed[16 * MIP_MAX_REDUCED];
  __shared__ int16_t sOrg[FUSED ? INTRA_MAX_AREA : 1], sPred[FUSED ? INTRA_MAX_AREA : 1];
  const int lanes = uni( *lanesPtr );
  if( ( long ) blockIdx.x * intra_chunk( lanes ) >= n ) return;
  const MipLds s = { sLine, sBdry, sIn, sRed, sOrg, sPred };
  constexpr MipOut OUT = FUSED ? MIP_OUT_DIST : MIP_OUT_PRED;
  if( lanes == 16 ) mip_chunk_body<16, OUT>( s, tab, refBase, orgBase, blocks, numBlocks, jobs, n, predBase, dist );
  else if( lanes == 64 ) mip_chunk_body<64, OUT>( s, tab, refBase, orgBase, blocks, numBlocks, jobs, n, predBase, dist );
  else mip_chunk_body<256, OUT>( s, tab, refBase, orgBase, blocks, numBlocks, jobs, n, predBase, dist );
}

int mip_launch( vtmhip_ctx *ctx, bool fused, const int16_t *d_refBase, const int16_t *d_orgBase, const vtmhip_intra_block *d_blocks, int numBlocks,
                const vtmhip_mip_job *d_jobs, int n, int16_t *d_predBase, uint64_t *d_dist )
{
  void *arena = nullptr;
  VTMHIP_TRY( vtmhip_internal_workspace( ctx, 256, &arena ) );
  int *d_lanes = ( int * ) arena;
  hipLaunchKernelGGL( intra_shape_kernel, dim3( 1 ), dim3( 256 ), 0, ctx->stream, d_blocks, numBlocks, d_lanes );
  VTMHIP_LAUNCHED( ctx );
  const dim3 grid( ( n + INTRA_MIN_CHUNK - 1 ) / INTRA_MIN_CHUNK );
  VTMHIP_TIME_KERNEL( ctx, fused ? "mip_presel_kernel" : "mip_pred_kernel" );
  if( fused )
    hipLaunchKernelGGL( mip_kernel<true>, grid, dim3( 256 ), 0, ctx->stream, d_lanes, ctx->mipTab, d_refBase, d_orgBase, d_blocks, numBlocks, d_jobs, n, d_predBase,
                        ( unsigned long long * ) d_dist );
  else
    hipLaunchKernelGGL( mip_kernel<false>, grid, dim3( 256 ), 0, ctx->stream, d_lanes, ctx->mipTab, d_refBase, d_orgBase, d_blocks, numBlocks, d_jobs, n, d_predBase,
                        ( unsigned long long * ) d_dist );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

}   // namespace

extern "C"
{

int vtmhip_mip_struct_size( int which ) { return which == 0 ? ( int ) sizeof( vtmhip_mip_job ) : -1; }

int vtmhip_mip_set_tables( vtmhip_ctx *ctx, const uint8_t *m4x4, const uint8_t *m8x8, const uint8_t *m16x16 )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, m4x4 && m8x8 && m16x16, "null table" );
  std::lock_guard<std::mutex> lock( ctx->initMutex );
  if( !ctx->mipTab ) VTMHIP_HIP( ctx, hipMalloc( ( void ** ) &ctx->mipTab, MIP_TAB_BYTES ) );
  VTMHIP_HIP( ctx, hipMemcpyAsync( ctx->mipTab, m4x4, MIP_BYTES_4X4, hipMemcpyHostToDevice, ctx->stream ) );
  VTMHIP_HIP( ctx, hipMemcpyAsync( ctx->mipTab + MIP_BYTES_4X4, m8x8, MIP_BYTES_8X8, hipMemcpyHostToDevice, ctx->stream ) );
  VTMHIP_HIP( ctx, hipMemcpyAsync( ctx->mipTab + MIP_BYTES_4X4 + MIP_BYTES_8X8, m16x16, MIP_BYTES_16X16, hipMemcpyHostToDevice, ctx->stream ) );
  VTMHIP_HIP( ctx, hipStreamSynchronize( ctx->stream ) );
  return VTMHIP_OK;
}

int vtmhip_mip_pred_host( int width, int height, int bitDepth, int mode, int transposed, const int16_t *top, const int16_t *left, const uint8_t *m4x4, const uint8_t *m8x8,
                          const uint8_t *m16x16, int16_t *pred )
{
  if( !top || !left || !m4x4 || !m8x8 || !m16x16 || !pred || !mipBlockOk( width, height, bitDepth, 0 ) || !mipJobOk( mipShape( width, height ), mode, transposed ) )
    return VTMHIP_E_INVALID;
  mipPredict( width, height, bitDepth, mode, transposed, top, left, m4x4, m8x8, m16x16, pred );
  return VTMHIP_OK;
}

int vtmhip_mip_pred_batch_dev( vtmhip_ctx *ctx, const int16_t *d_refBase, const vtmhip_intra_block *d_blocks, int numBlocks, const vtmhip_mip_job *d_jobs, int n,
                               int16_t *d_predBase )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, ctx->mipTab, "vtmhip_mip_set_tables has not been called" );
  VTMHIP_REQUIRE( ctx, numBlocks >= 0, "numBlocks" );
  VTMHIP_BATCH_ARGS( ctx, n, d_refBase && d_blocks && d_jobs && d_predBase );
  VTMHIP_REQUIRE( ctx, numBlocks > 0, "jobs without blocks" );
  return mip_launch( ctx, false, d_refBase, nullptr, d_blocks, numBlocks, d_jobs, n, d_predBase, nullptr );
}

int vtmhip_mip_presel_batch_dev( vtmhip_ctx *ctx, const int16_t *d_refBase, const int16_t *d_orgBase, const vtmhip_intra_block *d_blocks, int numBlocks,
                                 const vtmhip_mip_job *d_jobs, int n, uint64_t *d_dist )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, ctx->mipTab, "vtmhip_mip_set_tables has not been called" );
  VTMHIP_REQUIRE( ctx, numBlocks >= 0, "numBlocks" );
  VTMHIP_BATCH_ARGS( ctx, n, d_refBase && d_orgBase && d_blocks && d_jobs && d_dist );
  VTMHIP_REQUIRE( ctx, numBlocks > 0, "jobs without blocks" );
  return mip_launch( ctx, true, d_refBase, d_orgBase, d_blocks, numBlocks, d_jobs, n, nullptr, d_dist );
}

}   // extern "C"
