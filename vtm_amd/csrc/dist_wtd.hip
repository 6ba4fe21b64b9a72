// dist_wtd.hip -- luma-level-weighted SSE: RdCost::m_afpDistortFunc[DF_SSE_WTD .. DF_SSE16N_WTD] (RdCost::xGetSSE*_WTD, reference CommonLib/RdCost.cpp:3088-3463,
// per-sample rule RdCost::getWeightedMSE :3055-3086), the CU-level final distortion of LMCS / WCG encodes.  Bit-exact with the reference under the sample
// contract of include/vtmhip.h (org, cur, orgLuma in [0, 2^bitDepth), bitDepth <= 12), including the truncation of the weighted square to 32 bits.
//
// sse_wtd_kernel (4 waves per workgroup) packs jobs into waves as wave_pack.hpp lays out; an item is a 4-sample row segment, walked lane-strided:
//   - the fixed-point weight table (<= 4096 x int32) and the inverse reshape LUT (<= 4096 x int16) are staged in LDS once per workgroup with 16-byte loads;
//     every per-sample weight / inverse-LUT lookup is an LDS read;
//   - a lane accumulates in 64 bits while its segments belong to one job and adds the partial into the job's LDS slot when it moves on (integer sum:
//     order-free); the 64-bit weighted square is one 32 x 32 -> 64 multiply (fixed < 2^31, d * d < 2^24), never a generic 64 x 64 one.
#include "ctx.hpp"
#include "stage.hpp"
#include "wave_pack.hpp"
#include "pel_pack.hpp"

namespace
{

constexpr int WTD_WAVES = 4;     // waves per workgroup
constexpr int WTD_MAX_TAB = 4096;

struct WtdJobL   // a job as the kernel uses it (LDS, one per lane of a group)
{
  const int16_t *org, *cur, *luma;
  int os, cs, ls;
  int w;
  FastDiv segs;     // segment index -> (row, segment)
  int mode;         // bit 0: inverse-reshape cur; bit 1: chroma with the constant weight; bit 2: chroma weighted by the co-located luma; bits 8..: cShiftX | cShiftY << 1
};

__device__ __forceinline__ unsigned long long wmse( int fixed, int o, int c )
{
  const int      d  = o - c;
  const unsigned dd = ( unsigned ) d * ( unsigned ) d;                                                // < 2^24 under the sample contract
  const unsigned long long p = ( unsigned long long ) ( unsigned ) fixed * dd;                        // v_mul_lo_u32 + v_mul_hi_u32
  const int mse = ( int ) ( unsigned ) ( ( p + 32768ull ) >> 16 );                                   // Intermediate_Int( ... ): low 32 bits
  return ( unsigned long long ) ( long long ) mse;                                                    // Distortion( mse >> 0 )
}

__global__ __launch_bounds__( 64 * WTD_WAVES ) void sse_wtd_kernel( const int16_t *__restrict__ orgBase, const int16_t *__restrict__ curBase,
                                                                   const int16_t *__restrict__ lumaBase, const vtmhip_wtd_job *__restrict__ jobs, int n, int G,
                                                                   const int32_t *__restrict__ fixedTab, const int16_t *__restrict__ invTab, int tabN,
                                                                   int chromaFixed, int chromaConst, unsigned long long *__restrict__ out )
{
  extern __shared__ __attribute__( ( aligned( 16 ) ) ) int32_t sTab[];   // [tabN] fixed weights, then [tabN] int16 inverse LUT when invTab != nullptr
  __shared__ WtdJobL            sJob[WTD_WAVES][64];
  __shared__ int                sEnd[WTD_WAVES][64];   // inclusive prefix of the groups' segment counts
  __shared__ unsigned long long sSum[WTD_WAVES][64];
  int16_t *sInv = reinterpret_cast<int16_t *>( sTab + tabN );

  for( int i = threadIdx.x; i < ( tabN >> 2 ); i += blockDim.x ) reinterpret_cast<int4 *>( sTab )[i] = reinterpret_cast<const int4 *>( fixedTab )[i];
  if( invTab )
    for( int i = threadIdx.x; i < ( tabN >> 3 ); i += blockDim.x ) reinterpret_cast<int4 *>( sInv )[i] = reinterpret_cast<const int4 *>( invTab )[i];

  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, top = tabN - 1;
  const int nGroups = wave_groups( n, G );
  // every wave of a workgroup runs the same number of rounds (the barriers below)
  for( int round = blockIdx.x * WTD_WAVES; round < nGroups; round += gridDim.x * WTD_WAVES )
  {
    const WaveGroup g( round, wv, lane, n, G, nGroups );
    int  items = 0;
    bool valid = false;
    if( g.mine )
    {
      const vtmhip_wtd_job j = jobs[g.job];
      const int  w = j.width, h = j.height, comp = j.compID, sx = j.cShiftX, sy = j.cShiftY, fl = j.flags;
      const bool inv = ( fl & VTMHIP_WTD_INV_RESHAPE_CUR ) != 0;
      valid = w >= 1 && w <= 128 && h >= 1 && h <= 128 && comp <= 2 && sx <= 1 && sy <= 1 && ( comp != 0 || ( sx | sy ) == 0 ) &&
              ( fl & ~VTMHIP_WTD_INV_RESHAPE_CUR ) == 0 && ( !inv || ( comp == 0 && invTab ) );
      if( valid )
      {
        WtdJobL &L = sJob[wv][lane];
        L.org = orgBase + j.orgOff; L.cur = curBase + j.curOff; L.luma = lumaBase + j.orgLumaOff;
        L.os = j.orgStride; L.cs = j.curStride; L.ls = j.orgLumaStride;
        L.w = w; L.segs = FastDiv( ( w + 3 ) >> 2 );
        L.mode = ( inv ? 1 : 0 ) | ( comp != 0 ? ( chromaConst ? 2 : 4 ) : 0 ) | ( ( sx | sy << 1 ) << 8 );
        items = h * L.segs.d;
      }
    }
    const int total = wave_scan_items( lane, items, sEnd[wv] );
    sSum[wv][lane] = 0;
    __syncthreads();   // also orders the table staging of the first round

    // lane walks the group's segments t = lane, lane + 64, ...: its job index only grows
    WaveCursor         cur;
    WtdJobL            L {};
    unsigned long long acc = 0;
    for( int t = lane; t < total; t += 64 )
    {
      if( cur.beyond( t ) )
      {
        if( cur.cj >= 0 ) atomicAdd( &sSum[wv][cur.cj], acc );
        acc = 0;
        cur.advance( t, sEnd[wv] );
        L = sJob[wv][cur.cj];
      }
      const int local = t - cur.start, r = L.segs( local ), x = ( local - r * L.segs.d ) << 2, cnt = min( 4, L.w - x );
      const int16_t *o = L.org + ( long ) r * L.os + x, *c = L.cur + ( long ) r * L.cs + x;
      int            ov[4], cv[4];   // past the block's right edge org = cur = 0: d = 0 adds 0
      if( cnt == 4 ) { unpack4( *reinterpret_cast<const Pel4 *>( o ), ov ); unpack4( *reinterpret_cast<const Pel4 *>( c ), cv ); }   // one branch: both loads go out together
      else { ld4( o, cnt, ov ); ld4( c, cnt, cv ); }
      if( L.mode & 1 )
      {
#pragma unroll
        for( int k = 0; k < 4; k++ )
          if( x + k < L.w ) cv[k] = sInv[min( max( cv[k], 0 ), top )];   // past the right edge org = cur = 0 must stay equal
      }
      if( L.mode & 2 )
      {
#pragma unroll
        for( int k = 0; k < 4; k++ ) acc += wmse( chromaFixed, ov[k], cv[k] );
      }
      else if( L.mode & 4 )
      {
        const int      sx = ( L.mode >> 8 ) & 1, sy = ( L.mode >> 9 ) & 1;
        const int16_t *lr = L.luma + ( long ) ( r << sy ) * L.ls;
#pragma unroll
        for( int k = 0; k < 4; k++ )
        {
          const int lv = x + k < L.w ? lr[( x + k ) << sx] : 0;
          acc += wmse( sTab[min( max( lv, 0 ), top )], ov[k], cv[k] );
        }
      }
      else
      {
#pragma unroll
        for( int k = 0; k < 4; k++ ) acc += wmse( sTab[min( max( ov[k], 0 ), top )], ov[k], cv[k] );
      }
    }
    if( cur.cj >= 0 ) atomicAdd( &sSum[wv][cur.cj], acc );
    __syncthreads();
    if( g.mine ) out[g.job] = valid ? sSum[wv][lane] : ~0ull;
    __syncthreads();   // sJob / sEnd / sSum are rewritten by the next round
  }
}

int wtd_launch( vtmhip_ctx *ctx, const int16_t *d_orgBase, const int16_t *d_curBase, const int16_t *d_lumaBase, const vtmhip_wtd_job *d_jobs, int n, int G,
                unsigned long long *d_out )
{
  const int    tabN    = 1 << ctx->wtdLumaBD;
  const size_t lds     = ( size_t ) tabN * sizeof( int32_t ) + ( ctx->wtdHasInv ? ( size_t ) tabN * sizeof( int16_t ) : 0 );
  const int    blocks  = wave_blocks( n, G, WTD_WAVES, ctx->numCUs * 8 );   // the tables are staged once per workgroup
  const int chromaConst = ctx->wtdSignalType == 0 || ctx->wtdSignalType == 2;   // RESHAPE_SIGNAL_SDR / _HLG: m_chromaWeight (RdCost.cpp:3066-3076)
  VTMHIP_TIME_KERNEL( ctx, "sse_wtd_kernel" );
  hipLaunchKernelGGL( sse_wtd_kernel, dim3( blocks ), dim3( 64 * WTD_WAVES ), lds, ctx->stream, d_orgBase, d_curBase, d_lumaBase, d_jobs, n, G, ctx->wtdFixed,
                      ctx->wtdHasInv ? ctx->wtdInv : nullptr, tabN, ( int ) ctx->wtdChromaFixed, chromaConst, d_out );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

}   // namespace

extern "C"
{

int vtmhip_set_luma_level_weights( vtmhip_ctx *ctx, const double *lut, int lumaBD, int signalType, double chromaWeight, const int16_t *invLut )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, lut != nullptr, "null weight table" );
  VTMHIP_REQUIRE( ctx, lumaBD >= 8 && lumaBD <= 12, "lumaBD must be 8..12" );
  const int                  tabN = 1 << lumaBD;
  const double               lim  = 2147483648.0;   // the fixed weight times d * d (< 2^24) must stay inside the 32 x 32 -> 64 product
  std::vector<int32_t>       fx( tabN );
  for( int i = 0; i < tabN; i++ )
  {
    const double v = lut[i] * 65536.0;
    VTMHIP_REQUIRE( ctx, v >= 0.0 && v < lim, "a luma-level weight * 65536 is outside [0, 2^31)" );
    fx[i] = ( int32_t ) ( int64_t ) v;   // (int64_t)( weight * (double)( 1 << 16 ) ), RdCost.cpp:3082
  }
  const double cv = chromaWeight * 65536.0;
  VTMHIP_REQUIRE( ctx, cv >= 0.0 && cv < lim, "chromaWeight * 65536 is outside [0, 2^31)" );
  std::lock_guard<std::mutex> lock( ctx->initMutex );
  if( !ctx->wtdFixed ) VTMHIP_HIP( ctx, hipMalloc( ( void ** ) &ctx->wtdFixed, WTD_MAX_TAB * sizeof( int32_t ) ) );
  if( invLut && !ctx->wtdInv ) VTMHIP_HIP( ctx, hipMalloc( ( void ** ) &ctx->wtdInv, WTD_MAX_TAB * sizeof( int16_t ) ) );
  VTMHIP_HIP( ctx, hipMemcpyAsync( ctx->wtdFixed, fx.data(), tabN * sizeof( int32_t ), hipMemcpyHostToDevice, ctx->stream ) );
  if( invLut ) VTMHIP_HIP( ctx, hipMemcpyAsync( ctx->wtdInv, invLut, tabN * sizeof( int16_t ), hipMemcpyHostToDevice, ctx->stream ) );
  VTMHIP_HIP( ctx, hipStreamSynchronize( ctx->stream ) );   // fx and the caller's arrays may go away
  ctx->wtdLumaBD = lumaBD; ctx->wtdSignalType = signalType; ctx->wtdChromaFixed = ( int32_t ) ( int64_t ) cv; ctx->wtdHasInv = invLut != nullptr;
  return VTMHIP_OK;
}

int vtmhip_sse_wtd_batch_dev( vtmhip_ctx *ctx, const int16_t *d_orgBase, const int16_t *d_curBase, const int16_t *d_orgLumaBase, const vtmhip_wtd_job *d_jobs,
                              int n, uint64_t *d_dist )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, ctx->wtdLumaBD != 0, "vtmhip_set_luma_level_weights has not been called" );
  VTMHIP_BATCH_ARGS( ctx, n, d_orgBase && d_curBase && d_orgLumaBase && d_jobs && d_dist );
  return wtd_launch( ctx, d_orgBase, d_curBase, d_orgLumaBase, d_jobs, n, wave_jobs_per_wave( ctx->numCUs, n ), ( unsigned long long * ) d_dist );
}

int vtmhip_xGetSSE_WTD( vtmhip_ctx *ctx, const int16_t *org, int orgStride, const int16_t *cur, int curStride, int width, int height, int compID,
                        const int16_t *orgLuma, int orgLumaStride, int cShiftX, int cShiftY, uint64_t *dist )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, ctx->wtdLumaBD != 0, "vtmhip_set_luma_level_weights has not been called" );
  VTMHIP_REQUIRE( ctx, org && cur && dist, "null pointer" );
  VTMHIP_REQUIRE( ctx, width >= 1 && height >= 1 && width <= 128 && height <= 128, "block size must be 1..128" );
  VTMHIP_REQUIRE( ctx, compID >= 0 && compID <= 2, "compID must be 0..2" );
  VTMHIP_REQUIRE( ctx, cShiftX >= 0 && cShiftX <= 1 && cShiftY >= 0 && cShiftY <= 1 && ( compID != 0 || ( cShiftX | cShiftY ) == 0 ), "cShiftX / cShiftY" );
  const bool lumaW = compID != 0 && !( ctx->wtdSignalType == 0 || ctx->wtdSignalType == 2 );   // chroma weighted by the co-located luma level
  VTMHIP_REQUIRE( ctx, compID == 0 || orgLuma, "a chroma block needs orgLuma" );
  // stage org, cur and (chroma) the luma samples the block reads compactly: stride = width, luma rows of lw = ((width - 1) << cShiftX) + 1 samples
  const int    lw  = compID != 0 ? ( ( width - 1 ) << cShiftX ) + 1 : 1;
  HostStage    s( ctx );
  const size_t blk = ( size_t ) width * height * sizeof( int16_t ), lblk = ( size_t ) lw * height * sizeof( int16_t );
  const size_t orgOff = s.region( blk ), curOff = s.region( blk ), lumaOff = s.region( lblk ), jobOff = s.region( sizeof( vtmhip_wtd_job ) ), outOff = s.region( 8 );
  VTMHIP_TRY( s.reserve() );
  s.pack( orgOff, org, orgStride, width, height );
  for( int i = 0; i < width * height; i++ ) VTMHIP_REQUIRE( ctx, s.host<int16_t>( orgOff )[i] >= 0, "negative org sample (RdCost.cpp:3060: CHECK( org < 0 ))" );
  s.pack( curOff, cur, curStride, width, height );
  if( lumaW ) s.pack( lumaOff, orgLuma, ( ptrdiff_t ) orgLumaStride * ( 1 << cShiftY ), lw, height );
  vtmhip_wtd_job j;
  memset( &j, 0, sizeof( j ) );
  j.orgOff = ( int64_t ) ( orgOff / 2 ); j.curOff = ( int64_t ) ( curOff / 2 ); j.orgLumaOff = ( int64_t ) ( lumaOff / 2 );
  j.orgStride = width; j.curStride = width; j.orgLumaStride = lw;
  j.width = ( int16_t ) width; j.height = ( int16_t ) height; j.compID = ( uint8_t ) compID;
  j.cShiftX = ( uint8_t ) cShiftX; j.cShiftY = 0;   // the staged luma rows are already the (y << cShiftY) ones
  s.put( jobOff, j );
  VTMHIP_TRY( s.upload( 0, outOff ) );
  VTMHIP_TRY( wtd_launch( ctx, s.dev<const int16_t>( 0 ), s.dev<const int16_t>( 0 ), s.dev<const int16_t>( 0 ), s.dev<const vtmhip_wtd_job>( jobOff ), 1, 1,
                          s.dev<unsigned long long>( outOff ) ) );
  VTMHIP_TRY( s.fetch( outOff, 8 ) );
  memcpy( dist, s.hp + outOff, 8 );
  return VTMHIP_OK;
}

}   // extern "C"
