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
#include "ctx.hpp"
#include "dist_block.hpp"
#include "cclm_rules.hpp"

namespace
{

constexpr int ICH_LINE     = 72;     // 2 * 32 + 1 samples of a line, rounded up
constexpr int ICH_MAX_AREA = 1024;
constexpr int ICH_EDGE     = 64;     // the top row / left column of the down-sampled luma: up to 2 * 32
constexpr int ICH_MIN_CHUNK = 8;

__host__ __device__ inline int ich_lanes( int maxArea ) { return maxArea <= 64 ? 16 : 64; }
__host__ __device__ inline int ich_chunk( int lanes ) { return lanes == 16 ? 16 : 8; }

__host__ __device__ inline CclmAvail ich_avail( const vtmhip_intra_chroma_block &b )
{
  const CclmAvail v = { b.above, b.left, b.aboveRight, b.belowLeft, b.firstRow, b.colocated };
  return v;
}
__host__ __device__ inline bool ich_block_ok( const vtmhip_intra_chroma_block &b ) { return cclmBlockOk( b.width, b.height, b.bitDepth, ich_avail( b ) ); }

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

// the staged down-sampled luma as cclmModel reads it
struct IchDs
{
  const int16_t *top, *left;
  __host__ __device__ int operator()( int i, int j ) const { return j < 0 ? top[i] : left[j]; }
};

struct IchLds
{
  int16_t   *line;    // [4][ICH_LINE]: Cb top, Cb left, Cr top, Cr left
  int16_t   *ds;      // [ICH_MAX_AREA] inner, [ICH_EDGE] top, [ICH_EDGE] left
  CclmModel *model;   // [3 modes][2 components]
  int       *dc;      // [2]
  int16_t   *org, *pred;   // fused only: [2][ICH_MAX_AREA], [G][2][area]
};

template<int L, bool FUSED>
__device__ __forceinline__ void ich_chunk_body( const IchLds &s, const int16_t *__restrict__ refBase, const int16_t *__restrict__ lumaBase, const int16_t *__restrict__ orgBase,
                                                const vtmhip_intra_chroma_block *__restrict__ blocks, int numBlocks, const vtmhip_intra_chroma_job *__restrict__ jobs, int n,
                                                int16_t *__restrict__ predBase, unsigned long long *__restrict__ dist )
{
  constexpr int G = 256 / L, CHUNK = L == 16 ? 16 : 8;
  const int tid = threadIdx.x, g = tid / L, l = tid % L;
  const int jBegin = blockIdx.x * CHUNK, jEnd = min( n, jBegin + CHUNK );
  int16_t  *sDsTop = s.ds + ICH_MAX_AREA, *sDsLeft = sDsTop + ICH_EDGE;

  for( int j = jBegin; j < jEnd; )
  {
    // the run [j, e) of one block index (uniform over the workgroup)
    const int blk = uni( jobs[j].block );
    int       e   = j + 1;
    while( e < jEnd && uni( jobs[e].block ) == blk ) e++;
    const int first = j;
    j = e;
    if( blk < 0 || blk >= numBlocks ) continue;
    const vtmhip_intra_chroma_block B = blocks[blk];
    const int w = uni( ( int ) B.width ), h = uni( ( int ) B.height ), bd = uni( ( int ) B.bitDepth );
    CclmAvail V;
    V.above = uni( ( int ) B.above ); V.left = uni( ( int ) B.left ); V.aboveRight = uni( ( int ) B.aboveRight ); V.belowLeft = uni( ( int ) B.belowLeft );
    V.firstRow = uni( ( int ) B.firstRow ); V.colocated = uni( ( int ) B.colocated );
    if( !cclmBlockOk( w, h, bd, V ) || w * h > ( L == 16 ? 64 : ICH_MAX_AREA ) ) continue;   // the second part cannot happen: L comes from the largest block
    const int area = w * h, log2W = intraLog2( w ), log2H = intraLog2( h ), nTop = 2 * w + 1, nLeft = 2 * h + 1, maxVal = ( 1 << bd ) - 1;

    // does the run hold an LM job?  (a run has at most CHUNK <= 16 jobs)
    const int anyLm = __syncthreads_or( first + tid < e && cclmIsLm( jobs[first + tid].mode ) && cclmModeOk( jobs[first + tid].mode ) );   // also: the previous run's readers are done
    {
      const int nLine = nTop + nLeft;
      for( int i = tid; i < 2 * nLine; i += 256 )
      {
        const int c = i >= nLine, k = i - c * nLine;
        const int16_t v = refBase[( c ? B.crRefOff : B.cbRefOff ) + k];
        s.line[( 2 * c + ( k >= nTop ) ) * ICH_LINE + ( k >= nTop ? k - nTop : k )] = v;
      }
      if( FUSED )
        for( int i = tid; i < 2 * area; i += 256 )
        {
          const int c = i >= area, k = i - c * area;
          s.org[c * ICH_MAX_AREA + k] = orgBase[( c ? B.crOrgOff : B.cbOrgOff ) + ( long ) ( k >> log2W ) * B.orgStride + ( k & ( w - 1 ) )];
        }
      if( anyLm )
      {
        const CclmLuma luma = { lumaBase + B.lumaOff, B.lumaStride };
        const int reachT = cclmTopReach( w, h, V ), reachL = cclmLeftReach( w, h, V );
        for( int i = tid; i < area + reachT + reachL; i += 256 )
        {
          if( i < area ) s.ds[i] = ( int16_t ) cclmDsSample( luma, V, i & ( w - 1 ), i >> log2W );
          else if( i < area + reachT ) sDsTop[i - area] = ( int16_t ) cclmDsSample( luma, V, i - area, -1 );
          else sDsLeft[i - area - reachT] = ( int16_t ) cclmDsSample( luma, V, -1, i - area - reachT );
        }
      }
    }
    __syncthreads();
    IntraBlk U;   // of component c: the lines at ( 2 c, 2 c + 1 )
    U.w = w; U.h = h; U.log2W = log2W; U.log2H = log2H; U.m = 0; U.maxVal = maxVal;
    if( tid >= 254 || ( anyLm && tid < 6 ) )
    {
      const int c = tid & 1;
      U.top = s.line + 2 * c * ICH_LINE; U.left = U.top + ICH_LINE;
      if( tid >= 254 ) s.dc[c] = intraDcVal( U );
      else
      {
        const IchDs ds = { sDsTop, sDsLeft };
        s.model[tid] = cclmModel( w, h, CCLM_LM + ( tid >> 1 ), bd, V, U.top, U.left, ds );
      }
    }
    __syncthreads();

    for( int base = first; base < e; base += G )
    {
      const int job = base + g;
      bool      ok  = job < e;
      vtmhip_intra_chroma_job J;
      if( ok )
      {
        J  = jobs[job];
        ok = cclmModeOk( J.mode );
      }
      int16_t *slot = FUSED ? s.pred + g * 2 * area : nullptr;
      if( ok )
      {
        if( cclmIsLm( J.mode ) )
        {
          for( int i = l; i < 2 * area; i += L )
          {
            const int c = i >= area, k = i - c * area;
            const int16_t v = cclmPredSample( s.model[2 * ( J.mode - CCLM_LM ) + c], s.ds[k], maxVal );
            if( FUSED ) slot[i] = v;
            else predBase[( c ? J.crPredOff : J.cbPredOff ) + k] = v;
          }
        }
        else
        {
          vtmhip_intra_params p;
          intraPredParams( w, h, J.mode, 0, p, true );
          for( int i = l; i < 2 * area; i += L )
          {
            const int c = i >= area, k = i - c * area;
            U.top = s.line + 2 * c * ICH_LINE; U.left = U.top + ICH_LINE;
            const int16_t v = intraPredSample( p, J.mode, U, s.dc[c], nullptr, k & ( w - 1 ), k >> log2W, true );
            if( FUSED ) slot[i] = v;
            else predBase[( c ? J.crPredOff : J.cbPredOff ) + k] = v;
          }
        }
      }
      if( FUSED )
      {
        __syncthreads();
        if( ok )
        {
#pragma unroll 1
          for( int c = 0; c < 2; c++ )   // one copy of the two reductions
          {
            const unsigned long long sad  = lanes_block_dist<L>( VTMHIP_DIST_SAD, s.org + c * ICH_MAX_AREA, w, slot + c * area, w, w, h, 0, l );
            const unsigned long long satd = lanes_block_dist<L>( VTMHIP_DIST_SATD, s.org + c * ICH_MAX_AREA, w, slot + c * area, w, w, h, 0, l );
            if( l == 0 ) { dist[4 * ( long ) job + 2 * c] = sad; dist[4 * ( long ) job + 2 * c + 1] = satd; }
          }
        }
        __syncthreads();   // before the next round overwrites the slots
      }
    }
  }
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
  if( lanes == 16 ) ich_chunk_body<16, FUSED>( s, refBase, lumaBase, orgBase, blocks, numBlocks, jobs, n, predBase, dist );
  else ich_chunk_body<64, FUSED>( s, refBase, lumaBase, orgBase, blocks, numBlocks, jobs, n, predBase, dist );
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
