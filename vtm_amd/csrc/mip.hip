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
#include "ctx.hpp"
#include "dist_block.hpp"
#include "intra_lanes.hpp"
#include "mip_rules.hpp"

namespace
{

constexpr int MIP_LINE      = 72;   // indices 1 .. 64 of a line, rounded up
constexpr int MIP_TAB_BYTES = MIP_BYTES_4X4 + MIP_BYTES_8X8 + MIP_BYTES_16X16;

struct MipLds
{
  int16_t *line;   // [2][MIP_LINE]: top, left, indexed as the block's lines are (1 .. W, 1 .. H)
  int     *bdry;   // [2][4]: reduced top, reduced left
  int     *in;     // [2][MIP_MAX_INPUT]: the rebased input, top | left then left | top
  int16_t *red;    // [16][MIP_MAX_REDUCED]: a reduced block per lane group
  int16_t *org, *pred;   // fused only
};

template<int L, bool FUSED>
__device__ __forceinline__ void mip_chunk_body( const MipLds &s, const uint8_t *__restrict__ tab, const int16_t *__restrict__ refBase, const int16_t *__restrict__ orgBase,
                                                const vtmhip_intra_block *__restrict__ blocks, int numBlocks, const vtmhip_mip_job *__restrict__ jobs, int n,
                                                int16_t *__restrict__ predBase, unsigned long long *__restrict__ dist )
{
  constexpr int G = 256 / L, CHUNK = L == 16 ? 16 : L == 64 ? 8 : 4;
  const int tid = threadIdx.x, g = tid / L, l = tid % L;
  const int jBegin = blockIdx.x * CHUNK, jEnd = min( n, jBegin + CHUNK );
  int16_t  *sTop = s.line, *sLeft = s.line + MIP_LINE;

  for( int j = jBegin; j < jEnd; )
  {
    // the run [j, e) of one block index (uniform over the workgroup)
    const int blk = uni( jobs[j].block );
    int       e   = j + 1;
    while( e < jEnd && uni( jobs[e].block ) == blk ) e++;
    const int first = j;
    j = e;
    if( blk < 0 || blk >= numBlocks ) continue;
    const vtmhip_intra_block B = blocks[blk];
    const int w = uni( ( int ) B.width ), h = uni( ( int ) B.height ), m = uni( ( int ) B.multiRefIdx ), bd = uni( ( int ) B.bitDepth );
    if( !mipBlockOk( w, h, bd, m ) || w * h > ( L == 16 ? 64 : L == 64 ? 1024 : INTRA_MAX_AREA ) ) continue;   // the second part cannot happen: L comes from the largest block
    const MipShape S = mipShape( w, h );
    const int area = w * h, log2W = mipLog2( w ), nRed = S.pred * S.pred;

    __syncthreads();   // the previous run's readers are done
    {
      const int16_t *ref = refBase + B.refOff;   // top[i] = ref[i], left[i] = ref[2W + 1 + i]
      for( int i = tid; i < w + h; i += 256 )
      {
        if( i < w ) sTop[1 + i] = ref[1 + i];
        else sLeft[1 + i - w] = ref[2 * w + 2 + i - w];
      }
      if( FUSED )
      {
        const int16_t *org = orgBase + B.orgOff;
        for( int i = tid; i < area; i += 256 ) s.org[i] = org[( long ) ( i >> log2W ) * B.orgStride + ( i & ( w - 1 ) )];
      }
    }
    __syncthreads();
    if( tid < 2 * S.bdry )
    {
      const int t = tid >= S.bdry, i = tid - t * S.bdry;
      s.bdry[4 * t + i] = mipBoundarySample( t ? sLeft : sTop, t ? h : w, S.bdry, i );
    }
    __syncthreads();
    if( tid < 2 * MIP_MAX_INPUT && ( tid & 7 ) < 2 * S.bdry )
    {
      const int t = tid >> 3;   // 0: top | left, 1: left | top
      s.in[tid] = mipInputAt( S, bd, s.bdry + 4 * t, s.bdry + 4 * ( 1 - t ), tid & 7 );
    }
    __syncthreads();

    for( int base = first; base < e; base += G )
    {
      const int job = base + g;
      bool      ok  = job < e;
      vtmhip_mip_job J;
      if( ok )
      {
        J  = jobs[job];
        ok = mipJobOk( S, J.mode, J.transposed );
      }
      int16_t *red = s.red + g * MIP_MAX_REDUCED, *slot = FUSED ? s.pred + g * area : nullptr;
      if( ok )
      {
        const int      t      = J.transposed;
        const uint8_t *matrix = mipMatrix( S, J.mode, tab, tab + MIP_BYTES_4X4, tab + MIP_BYTES_4X4 + MIP_BYTES_8X8 );
        for( int pos = l; pos < nRed; pos += L ) red[mipRedIndex( S, t, pos )] = ( int16_t ) mipReducedSample( S, s.in + MIP_MAX_INPUT * t, s.bdry[4 * t], bd, matrix, pos );
      }
      __syncthreads();
      if( ok )
      {
        int16_t *out = FUSED ? slot : predBase + J.predOff;
        for( int i = l; i < area; i += L ) out[i] = mipSample( S, red, sTop, sLeft, i & ( w - 1 ), i >> log2W );
      }
      __syncthreads();   // the reduced blocks are free again; fused: the slots are complete
      if( FUSED )
      {
        if( L == 256 )
        {
          const int wv = tid >> 6;   // wave 0: SAD, wave 1: SATD
          if( ok && wv < 2 )
          {
            const unsigned long long d = wave_block_dist( wv ? VTMHIP_DIST_SATD : VTMHIP_DIST_SAD, s.org, w, slot, w, w, h, 0, tid & 63 );
            if( ( tid & 63 ) == 0 ) dist[2 * ( long ) job + wv] = d;
          }
        }
        else if( ok )
        {
          const unsigned long long sad  = lanes_block_dist<L>( VTMHIP_DIST_SAD, s.org, w, slot, w, w, h, 0, l );
          const unsigned long long satd = lanes_block_dist<L>( VTMHIP_DIST_SATD, s.org, w, slot, w, w, h, 0, l );
          if( l == 0 ) { dist[2 * ( long ) job] = sad; dist[2 * ( long ) job + 1] = satd; }
        }
        __syncthreads();   // before the next round overwrites the slots
      }
    }
  }
}

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
  if( lanes == 16 ) mip_chunk_body<16, FUSED>( s, tab, refBase, orgBase, blocks, numBlocks, jobs, n, predBase, dist );
  else if( lanes == 64 ) mip_chunk_body<64, FUSED>( s, tab, refBase, orgBase, blocks, numBlocks, jobs, n, predBase, dist );
  else mip_chunk_body<256, FUSED>( s, tab, refBase, orgBase, blocks, numBlocks, jobs, n, predBase, dist );
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
