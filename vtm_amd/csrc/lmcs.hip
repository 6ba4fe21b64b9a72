// lmcs.hip -- the simple LMCS (luma mapping with chroma scaling) sample ops of the residual path:
//   AreaBuf<Pel>::rspSignal / scaleSignal (reference CommonLib/Buffer.cpp:399-464) as pointer entries and as a batched scaleSignal,
//   the mapped-domain luma residual  resi = fwdLUT[org] - fwdLUT[pred]        (EncoderLib/InterSearch.cpp:7285-7296)
//   and the reconstruction           reco = clip( fwdLUT[pred] + resi )        (InterSearch.cpp:7540-7551).
// The scaling arithmetic is lmcs.hpp's; the chains with the scaling fused in are in transform.hip / jccr.hip.
//
// lmcs_op_kernel (4 waves per workgroup) packs jobs into waves as wave_pack.hpp lays out; an item is a 4-sample row segment (pel_pack.hpp's ld4 / st4), walked
// lane-strided.  The forward LUT (<= 4096 x int16) is staged in LDS once per workgroup with 16-byte loads; every lookup is an LDS read with the index clamped.
#include "ctx.hpp"
#include "stage.hpp"
#include "wave_pack.hpp"
#include "pel_pack.hpp"
#include "lmcs.hpp"

namespace
{

constexpr int LM_WAVES = 4;
constexpr int LM_MAX_TAB = 4096;
enum { OP_SCALE = 0, OP_RESI = 1, OP_RECO = 2 };

struct LmJobL   // a job as the kernel uses it (LDS, one per lane of a group)
{
  const int16_t *a, *b;   // SCALE: src, -;  RESI: org, pred;  RECO: pred, resi
  int16_t       *o, *o2;  // SCALE: dst, -;  RESI: resi, mapped prediction;  RECO: reco, -
  int       as, bs, os, o2s;
  int       w;
  FastDiv   segs;         // segment index -> (row, segment)
  int       mode;         // SCALE: dir;  RESI / RECO: VTMHIP_LMCS_* flags
  LmcsScale sc;
  int       maxAbs;       // SCALE: (1 << bitDepth) - 1;  RECO: the clip's upper bound
};

template<int OP>
__device__ __forceinline__ bool lm_job( const void *jobs, int job, const int16_t *aBase, const int16_t *bBase, int16_t *oBase, int16_t *o2Base, LmJobL &L, int &h )
{
  if( OP == OP_SCALE )
  {
    const vtmhip_scale_job j = reinterpret_cast<const vtmhip_scale_job *>( jobs )[job];
    if( !( j.width >= 1 && j.width <= 128 && j.height >= 1 && j.height <= 128 && j.scale >= 1 && j.scale <= 32767 && j.dir <= 1 && j.bitDepth >= 8 && j.bitDepth <= 12 ) ) return false;
    if( j.dir && j.width == 1 ) return false;   // the reference THROWs
    L.a = aBase + j.srcOff; L.b = nullptr; L.o = oBase + j.dstOff; L.o2 = nullptr;
    L.as = j.srcStride; L.bs = 0; L.os = j.dstStride; L.o2s = 0;
    L.w = j.width; h = j.height; L.mode = j.dir; L.sc = lmcs_scale_of( j.scale ); L.maxAbs = ( 1 << j.bitDepth ) - 1;
    return true;
  }
  const vtmhip_lmcs_job j = reinterpret_cast<const vtmhip_lmcs_job *>( jobs )[job];
  if( !( j.width >= 1 && j.width <= 128 && j.height >= 1 && j.height <= 128 ) ) return false;
  if( OP == OP_RESI )
  {
    if( j.flags & ~( VTMHIP_LMCS_MAP_PRED | VTMHIP_LMCS_WRITE_MAPPED ) ) return false;
    if( ( j.flags & VTMHIP_LMCS_WRITE_MAPPED ) && !o2Base ) return false;
    L.a = aBase + j.orgOff; L.b = bBase + j.predOff; L.o = oBase + j.resiOff; L.o2 = ( j.flags & VTMHIP_LMCS_WRITE_MAPPED ) ? o2Base + j.dstOff : nullptr;
    L.as = j.orgStride; L.bs = j.predStride; L.os = j.resiStride; L.o2s = j.dstStride;
    L.maxAbs = 0;
  }
  else
  {
    if( ( j.flags & ~VTMHIP_LMCS_MAP_PRED ) || j.bitDepth < 8 || j.bitDepth > 12 ) return false;
    L.a = aBase + j.predOff; L.b = bBase + j.resiOff; L.o = oBase + j.dstOff; L.o2 = nullptr;
    L.as = j.predStride; L.bs = j.resiStride; L.os = j.dstStride; L.o2s = 0;
    L.maxAbs = ( 1 << j.bitDepth ) - 1;
  }
  L.w = j.width; h = j.height; L.mode = j.flags; L.sc.scale = L.sc.magic = 0;
  return true;
}

template<int OP>
__global__ __launch_bounds__( 64 * LM_WAVES ) void lmcs_op_kernel( const int16_t *aBase, const int16_t *bBase, int16_t *oBase, int16_t *o2Base,
                                                                  const void *__restrict__ jobs, int n, int G, const int16_t *__restrict__ lut, int tabN )
{
  extern __shared__ __attribute__( ( aligned( 16 ) ) ) int16_t sLut[];   // [tabN] forward LUT (RESI / RECO)
  __shared__ LmJobL sJob[LM_WAVES][64];
  __shared__ int    sEnd[LM_WAVES][64];   // inclusive prefix of the groups' segment counts

  if( OP != OP_SCALE )
    for( int i = threadIdx.x; i < ( tabN >> 3 ); i += blockDim.x ) reinterpret_cast<int4 *>( sLut )[i] = reinterpret_cast<const int4 *>( lut )[i];

  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, top = tabN - 1;
  const int nGroups = wave_groups( n, G );
  // every wave of a workgroup runs the same number of rounds (the barriers below)
  for( int round = blockIdx.x * LM_WAVES; round < nGroups; round += gridDim.x * LM_WAVES )
  {
    const WaveGroup g( round, wv, lane, n, G, nGroups );
    int             items = 0;
    if( g.mine )
    {
      LmJobL L;
      int    h = 0;
      if( lm_job<OP>( jobs, g.job, aBase, bBase, oBase, o2Base, L, h ) )
      {
        L.segs = FastDiv( ( L.w + 3 ) >> 2 );
        sJob[wv][lane] = L;
        items = h * L.segs.d;
      }
    }
    const int total = wave_scan_items( lane, items, sEnd[wv] );
    __syncthreads();   // also orders the table staging of the first round

    // lane walks the group's segments t = lane, lane + 64, ...: its job index only grows
    WaveCursor cur;
    LmJobL     L {};
    for( int t = lane; t < total; t += 64 )
    {
      if( cur.beyond( t ) ) { cur.advance( t, sEnd[wv] ); L = sJob[wv][cur.cj]; }
      const int local = t - cur.start, r = L.segs( local ), x = ( local - r * L.segs.d ) << 2, cnt = min( 4, L.w - x );
      int       av[4], bv[4], ov[4];
      ld4( L.a + ( long ) r * L.as + x, cnt, av );
      if( OP == OP_SCALE )
      {
#pragma unroll
        for( int k = 0; k < 4; k++ ) ov[k] = L.mode ? lmcs_fwd( av[k], L.sc, L.maxAbs ) : lmcs_inv( av[k], ( int ) L.sc.scale, L.maxAbs );
      }
      else
      {
        ld4( L.b + ( long ) r * L.bs + x, cnt, bv );
        int *pred = OP == OP_RESI ? bv : av;
        if( L.mode & VTMHIP_LMCS_MAP_PRED )
        {
#pragma unroll
          for( int k = 0; k < 4; k++ ) pred[k] = sLut[min( max( pred[k], 0 ), top )];
        }
        if( OP == OP_RESI )
        {
#pragma unroll
          for( int k = 0; k < 4; k++ ) ov[k] = ( int ) sLut[min( max( av[k], 0 ), top )] - bv[k];   // Pel wrap at the store
          if( L.o2 ) st4( L.o2 + ( long ) r * L.o2s + x, cnt, bv );
        }
        else
        {
#pragma unroll
          for( int k = 0; k < 4; k++ ) ov[k] = min( L.maxAbs, max( 0, av[k] + bv[k] ) );
        }
      }
      st4( L.o + ( long ) r * L.os + x, cnt, ov );
    }
    __syncthreads();   // sJob / sEnd are rewritten by the next round
  }
}

// buf[i] = lut[buf[i]] on a compact block (the pointer entry).  The host has checked every sample against the table; the clamp only keeps the kernel from
// reading outside it should that check ever change.
__global__ __launch_bounds__( 256 ) void rsp_kernel( int16_t *__restrict__ buf, int count, const int16_t *__restrict__ lut, int lutSize )
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if( i < count ) buf[i] = lut[min( max( ( int ) buf[i], 0 ), lutSize - 1 )];
}

template<int OP>
int lm_launch( vtmhip_ctx *ctx, const int16_t *a, const int16_t *b, int16_t *o, int16_t *o2, const void *d_jobs, int n, int G )
{
  const int    tabN    = OP == OP_SCALE ? 0 : 1 << ctx->lmcsLumaBD;
  const size_t lds     = ( size_t ) tabN * sizeof( int16_t );
  const int    blocks  = wave_blocks( n, G, LM_WAVES, ctx->numCUs * 8 );   // the table is staged once per workgroup
  VTMHIP_TIME_KERNEL( ctx, "lmcs_op_kernel" );
  hipLaunchKernelGGL( lmcs_op_kernel<OP>, dim3( blocks ), dim3( 64 * LM_WAVES ), lds, ctx->stream, a, b, o, o2, d_jobs, n, G, ( const int16_t * ) ctx->lmcsFwd, tabN );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

}   // namespace

extern "C"
{

int vtmhip_lmcs_struct_size( int which )
{
  switch( which )
  {
  case 0: return ( int ) sizeof( vtmhip_lmcs_job );
  case 1: return ( int ) sizeof( vtmhip_scale_job );
  default: return -1;
  }
}

int vtmhip_set_lmcs_fwd_lut( vtmhip_ctx *ctx, const int16_t *fwdLut, int lumaBD )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, fwdLut != nullptr, "null forward LUT" );
  VTMHIP_REQUIRE( ctx, lumaBD >= 8 && lumaBD <= 12, "lumaBD must be 8..12" );
  std::lock_guard<std::mutex> lock( ctx->initMutex );
  if( !ctx->lmcsFwd ) VTMHIP_HIP( ctx, hipMalloc( ( void ** ) &ctx->lmcsFwd, LM_MAX_TAB * sizeof( int16_t ) ) );
  VTMHIP_HIP( ctx, hipMemcpyAsync( ctx->lmcsFwd, fwdLut, ( ( size_t ) 1 << lumaBD ) * sizeof( int16_t ), hipMemcpyHostToDevice, ctx->stream ) );
  VTMHIP_HIP( ctx, hipStreamSynchronize( ctx->stream ) );   // the caller's array may go away
  ctx->lmcsLumaBD = lumaBD;
  return VTMHIP_OK;
}

int vtmhip_rspSignal( vtmhip_ctx *ctx, int16_t *buf, int stride, int width, int height, const int16_t *lut, int lutSize )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, buf && lut, "null pointer" );
  VTMHIP_REQUIRE( ctx, width >= 1 && height >= 1 && width <= 128 && height <= 128, "block size must be 1..128" );
  VTMHIP_REQUIRE( ctx, lutSize >= 1 && lutSize <= 65536, "lutSize: 1 .. 65536" );
  HostStage    s( ctx );
  const int    count = width * height;
  const size_t blk = ( size_t ) count * sizeof( int16_t ), lutBytes = ( size_t ) lutSize * sizeof( int16_t ), bufOff = s.region( blk ), lutOff = s.region( lutBytes );
  VTMHIP_TRY( s.reserve() );
  s.pack( bufOff, buf, stride, width, height );
  for( int i = 0; i < count; i++ ) VTMHIP_REQUIRE( ctx, s.host<int16_t>( bufOff )[i] >= 0 && s.host<int16_t>( bufOff )[i] < lutSize, "a sample lies outside the LUT" );
  memcpy( s.hp + lutOff, lut, lutBytes );
  VTMHIP_TRY( s.upload( 0, lutOff + lutBytes ) );
  VTMHIP_TIME_KERNEL( ctx, "rsp_kernel" );
  hipLaunchKernelGGL( rsp_kernel, dim3( ( count + 255 ) / 256 ), dim3( 256 ), 0, ctx->stream, s.dev<int16_t>( bufOff ), count, s.dev<const int16_t>( lutOff ), lutSize );
  VTMHIP_LAUNCHED( ctx );
  VTMHIP_TRY( s.fetch( bufOff, blk ) );
  s.unpack( buf, stride, bufOff, width, height );
  return VTMHIP_OK;
}

int vtmhip_scaleSignal( vtmhip_ctx *ctx, int16_t *buf, int stride, int width, int height, int scale, int dir, int bitDepth )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, buf != nullptr, "null pointer" );
  VTMHIP_REQUIRE( ctx, width >= 1 && height >= 1 && width <= 128 && height <= 128, "block size must be 1..128" );
  VTMHIP_REQUIRE( ctx, scale >= 1 && scale <= 32767, "scale: 1 .. 32767" );
  VTMHIP_REQUIRE( ctx, bitDepth >= 8 && bitDepth <= 12, "bitDepth must be 8..12" );
  VTMHIP_REQUIRE( ctx, !( dir && width == 1 ), "forward scaling of a block of width 1 (Buffer.cpp:427: THROW)" );
  HostStage    s( ctx );
  const size_t blk = ( size_t ) width * height * sizeof( int16_t ), bufOff = s.region( blk ), jobOff = s.region( sizeof( vtmhip_scale_job ) );
  VTMHIP_TRY( s.reserve() );
  s.pack( bufOff, buf, stride, width, height );
  vtmhip_scale_job j;
  memset( &j, 0, sizeof( j ) );
  j.srcOff = j.dstOff = ( int64_t ) ( bufOff / 2 );
  j.srcStride = j.dstStride = width; j.width = ( int16_t ) width; j.height = ( int16_t ) height;
  j.scale = ( uint16_t ) scale; j.dir = dir ? 1 : 0; j.bitDepth = ( uint8_t ) bitDepth;
  s.put( jobOff, j );
  VTMHIP_TRY( s.upload( 0, s.total ) );
  VTMHIP_TRY( lm_launch<OP_SCALE>( ctx, s.dev<const int16_t>( 0 ), nullptr, s.dev<int16_t>( 0 ), nullptr, s.dev<void>( jobOff ), 1, 1 ) );
  VTMHIP_TRY( s.fetch( bufOff, blk ) );
  s.unpack( buf, stride, bufOff, width, height );
  return VTMHIP_OK;
}

int vtmhip_scale_signal_batch_dev( vtmhip_ctx *ctx, const int16_t *d_srcBase, int16_t *d_dstBase, const vtmhip_scale_job *d_jobs, int n )
{
  VTMHIP_BATCH_ENTRY( ctx, n, d_srcBase && d_dstBase && d_jobs );
  return lm_launch<OP_SCALE>( ctx, d_srcBase, nullptr, d_dstBase, nullptr, d_jobs, n, wave_jobs_per_wave( ctx->numCUs, n ) );
}

int vtmhip_lmcs_resi_batch_dev( vtmhip_ctx *ctx, const int16_t *d_orgBase, const int16_t *d_predBase, int16_t *d_resiBase, int16_t *d_dstBase,
                                const vtmhip_lmcs_job *d_jobs, int n )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, ctx->lmcsLumaBD != 0, "vtmhip_set_lmcs_fwd_lut has not been called" );
  VTMHIP_BATCH_ARGS( ctx, n, d_orgBase && d_predBase && d_resiBase && d_jobs );
  return lm_launch<OP_RESI>( ctx, d_orgBase, d_predBase, d_resiBase, d_dstBase, d_jobs, n, wave_jobs_per_wave( ctx->numCUs, n ) );
}

int vtmhip_lmcs_reco_batch_dev( vtmhip_ctx *ctx, const int16_t *d_predBase, const int16_t *d_resiBase, int16_t *d_dstBase, const vtmhip_lmcs_job *d_jobs, int n )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, ctx->lmcsLumaBD != 0, "vtmhip_set_lmcs_fwd_lut has not been called" );
  VTMHIP_BATCH_ARGS( ctx, n, d_predBase && d_resiBase && d_dstBase && d_jobs );
  return lm_launch<OP_RECO>( ctx, d_predBase, d_resiBase, d_dstBase, nullptr, d_jobs, n, wave_jobs_per_wave( ctx->numCUs, n ) );
}

}   // extern "C"
