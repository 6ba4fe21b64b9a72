// wp.hip -- explicit weighted prediction: the distortions of DistParam::applyWeight (RdCostWeightPrediction::xGetSADw / xGetSSEw / xGetHADsw, reference
// CommonLib/RdCostWeightPrediction.cpp:56-640, U0040_MODIFIED_WEIGHTEDPREDICTION_WITH_BIPRED_AND_CLIPPING = 1) and the sample ops WeightPrediction::addWeightUni /
// addWeightBi (WeightPrediction.cpp:46-64, 157-226, 288-392).  Bit-exact with the scalar reference under the sample contract of include/vtmhip.h.
// DISTORTION_PRECISION_ADJUSTMENT is 0 (FULL_NBIT, TypeDef.h:225-237): the reference's final `>> distortionShift` is a no-op and is left out.
//
// wp_dist_kernel (4 waves per workgroup) packs jobs into waves as wave_pack.hpp lays out, walked in wave-uniform steps of 64 items:
//   - an item is one row of a SAD / SSE job, one Hadamard tile of a HAD job (8x8, 4x4, or one step of the 2x2 row walk);
//   - the weighting is applied as the samples are loaded; a lane produces one 64-bit sum per item;
//   - the items of a job lie on consecutive lanes in increasing row / tile order, so a segmented inclusive scan over the lanes (keyed by the job), carried
//     from one 64-item step to the next through lane 63, gives every item the prefix sum of its job.  SADw's per-row early exit returns the FIRST prefix
//     that exceeds maxDist (row sums are >= 0: the prefixes never decrease), else the total: exactly one lane per job stores the result;
//   - the Hadamard tiles run in 32-bit integers (|diff| < 2^17: the packed 16-bit butterflies of had.hpp do not apply, and xCalcHADs8x8w has no DC
//     adjustment); integer sums, so the butterfly order does not change a result.
//
// wp_pred_kernel: one wave per job, 4-sample row segments over the lanes.
#include "ctx.hpp"
#include "stage.hpp"
#include "wave_pack.hpp"
#include "pel_pack.hpp"

namespace
{

constexpr int WP_WAVES = 4;   // waves per workgroup

// the sample contract of include/vtmhip.h (shared by the pointer entries, which check it on the host, and the kernels, which reject a job with it)
__host__ __device__ inline bool wp_param_ok( int w, int offset, int shift, int round )
{
  return w >= -256 && w <= 256 && shift >= 0 && shift <= 8 && offset >= -32768 && offset <= 32767 && round >= -32768 && round <= 32767;
}

__host__ __device__ inline bool wp_dist_ok( int width, int height, int kind, int bitDepth, int isBiPred, const vtmhip_wp_param &p )
{
  if( width < 1 || width > 128 || height < 1 || height > 128 || kind < 0 || kind > 2 || bitDepth < 8 || bitDepth > 12 || isBiPred < 0 || isBiPred > 1 ) return false;
  if( !wp_param_ok( p.w, p.offset, p.shift, p.round ) ) return false;
  const bool tiles = ( ( width | height ) & 3 ) == 0;   // the 8x8 or the 4x4 path
  return kind != VTMHIP_DIST_SATD || tiles || ( ( width | height ) & 1 ) == 0;
}

__host__ __device__ inline bool wp_pred_ok( const vtmhip_wp_pred_job &j )
{
  return j.width >= 1 && j.width <= 128 && j.height >= 1 && j.height <= 128 && j.bitDepth >= 8 && j.bitDepth <= 12 && j.mode <= VTMHIP_WP_BI &&
         wp_param_ok( j.w0, j.offset, j.shift, 0 ) && ( j.mode == VTMHIP_WP_UNI || wp_param_ok( j.w1, 0, 0, 0 ) );
}

// the prediction a distortion compares against, per sample (cur -> pred):
enum
{
  WPM_PLAIN    = 0,   // SADw, default weight, no offset: cur
  WPM_ADD      = 1,   // SADw, default weight, offset, bi: cur + offset (int: no clip, no Pel)
  WPM_ADD_CLIP = 2,   // SADw, default weight, offset, uni: ClipPel( cur + offset )
  WPM_PEL      = 3,   // SADw / SSEw bi, HADsw: Pel( ((w * cur + round) >> shift) + offset ), truncated to int16
  WPM_CLIP     = 4    // SADw / SSEw uni: ClipPel( ((w * cur + round) >> shift) + offset )
};

struct WpJobL   // a job as the kernel uses it (LDS, one per lane of a group)
{
  const int16_t *org, *cur;
  int os, cs;
  int w, kind, mode, cmax;
  int wt, off, sh, rnd;
  int tile;             // HAD: tile size 8 / 4 / 2
  FastDiv tpr;          // HAD: tiles per row: item -> (tile row, tile column)
  unsigned long long maxDist;
};

__device__ __forceinline__ int wp_pred( const WpJobL &L, int c )
{
  const int q = ( ( L.wt * c + L.rnd ) >> L.sh ) + L.off;
  switch( L.mode )
  {
  case WPM_PLAIN: return c;
  case WPM_ADD: return c + L.off;
  case WPM_ADD_CLIP: return min( max( c + L.off, 0 ), L.cmax );
  case WPM_PEL: return ( int16_t ) q;
  default: return min( max( q, 0 ), L.cmax );
  }
}

// one row of SADw / SSEw
__device__ __forceinline__ unsigned long long wp_row( const WpJobL &L, int r )
{
  const int16_t     *o = L.org + ( long ) r * L.os, *c = L.cur + ( long ) r * L.cs;
  const bool         sse = L.kind == VTMHIP_DIST_SSE;
  unsigned long long s = 0;
  int                x = 0;
  for( ; x + 4 <= L.w; x += 4 )
  {
    int ov[4], cv[4];
    ld4( o + x, 4, ov );
    ld4( c + x, 4, cv );
#pragma unroll
    for( int k = 0; k < 4; k++ )
    {
      const int d = ov[k] - wp_pred( L, cv[k] );
      if( sse )
      {
        const int rsd = ( int16_t ) d;   // Pel residual
        s += ( unsigned ) ( rsd * rsd );
      }
      else s += ( unsigned ) abs( d );
    }
  }
  for( ; x < L.w; x++ )
  {
    const int d = o[x] - wp_pred( L, c[x] );
    if( sse )
    {
      const int rsd = ( int16_t ) d;
      s += ( unsigned ) ( rsd * rsd );
    }
    else s += ( unsigned ) abs( d );
  }
  return s;
}

// in-place 1-D Hadamard butterflies of N values (any order: integer sums)
template<int N> __device__ __forceinline__ void hadamard( int *v, int stride )
{
#pragma unroll
  for( int len = 1; len < N; len <<= 1 )
#pragma unroll
    for( int i = 0; i < N; i += len << 1 )
#pragma unroll
      for( int j = i; j < i + len; j++ )
      {
        const int a = v[j * stride], b = v[( j + len ) * stride];
        v[j * stride] = a + b; v[( j + len ) * stride] = a - b;
      }
}

// one N x N tile (N = 8: xCalcHADs8x8w, (s + 2) >> 2; N = 4: xCalcHADs4x4w, (s + 1) >> 1) with its top-left sample at (x0, y0)
template<int N> __device__ __forceinline__ unsigned long long wp_had_tile( const WpJobL &L, int y0, int x0 )
{
  int d[N * N];
#pragma unroll
  for( int y = 0; y < N; y++ )
  {
    const int16_t *o = L.org + ( long ) ( y0 + y ) * L.os + x0, *c = L.cur + ( long ) ( y0 + y ) * L.cs + x0;
#pragma unroll
    for( int k = 0; k < N; k += 4 )
    {
      int ov[4], cv[4];
      ld4( o + k, 4, ov );
      ld4( c + k, 4, cv );
#pragma unroll
      for( int i = 0; i < 4; i++ ) d[y * N + k + i] = ov[i] - ( int16_t ) ( ( ( L.wt * cv[i] + L.rnd ) >> L.sh ) + L.off );   // Pel pred, never clipped
    }
    hadamard<N>( d + y * N, 1 );   // the row transform as the row arrives
  }
#pragma unroll
  for( int x = 0; x < N; x++ ) hadamard<N>( d + x, N );
  unsigned s = 0;
#pragma unroll
  for( int i = 0; i < N * N; i++ ) s += ( unsigned ) abs( d[i] );
  return N == 8 ? ( s + 2 ) >> 2 : ( s + 1 ) >> 1;
}

// step k of xGetHADsw's 2x2 path at column x0: the reference's y += 2 loop advances org / cur by ONE row per step (RdCostWeightPrediction.cpp:624-633),
// so step k reads rows k and k + 1 (not 2k and 2k + 1); xCalcHADs2x2w has no normalisation
__device__ __forceinline__ unsigned long long wp_had_2x2( const WpJobL &L, int k, int x0 )
{
  int d[4];
#pragma unroll
  for( int i = 0; i < 4; i++ )
  {
    const int r = k + ( i >> 1 ), x = x0 + ( i & 1 );
    d[i] = L.org[( long ) r * L.os + x] - ( int16_t ) ( ( ( L.wt * L.cur[( long ) r * L.cs + x] + L.rnd ) >> L.sh ) + L.off );
  }
  const int m0 = d[0] + d[2], m1 = d[1] + d[3], m2 = d[0] - d[2], m3 = d[1] - d[3];
  return ( unsigned ) ( abs( m0 + m1 ) + abs( m0 - m1 ) + abs( m2 + m3 ) + abs( m2 - m3 ) );
}

__device__ __forceinline__ unsigned long long wp_item( const WpJobL &L, int local )
{
  if( L.kind != VTMHIP_DIST_SATD ) return wp_row( L, local );
  const int ty = L.tpr( local ), tx = local - ty * L.tpr.d;
  if( L.tile == 8 ) return wp_had_tile<8>( L, ty << 3, tx << 3 );
  if( L.tile == 4 ) return wp_had_tile<4>( L, ty << 2, tx << 2 );
  return wp_had_2x2( L, ty, tx << 1 );
}

// 4 waves per SIMD: the 8x8 tile's 64 differences fit in 124 VGPRs without scratch (unbounded, the compiler takes 135; at 5 it spills)
__global__ __launch_bounds__( 64 * WP_WAVES, 4 ) void wp_dist_kernel( const int16_t *__restrict__ orgBase, const int16_t *__restrict__ curBase,
                                                                  const vtmhip_wp_dist_job *__restrict__ jobs, int n, int G, unsigned long long *__restrict__ out )
{
  __shared__ WpJobL sJob[WP_WAVES][64];
  __shared__ int    sEnd[WP_WAVES][64];   // inclusive prefix of the group's item counts

  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int nGroups = wave_groups( n, G );
  // every wave of a workgroup runs the same number of rounds (the barriers below)
  for( int round = blockIdx.x * WP_WAVES; round < nGroups; round += gridDim.x * WP_WAVES )
  {
    const WaveGroup g( round, wv, lane, n, G, nGroups );
    int items = 0;
    if( g.mine )
    {
      const vtmhip_wp_dist_job j = jobs[g.job];
      const int w = j.width, h = j.height, kind = j.kind;
      if( wp_dist_ok( w, h, kind, j.bitDepth, j.isBiPred, j.wp ) )
      {
        WpJobL &L = sJob[wv][lane];
        L.org = orgBase + j.orgOff; L.cur = curBase + j.curOff; L.os = j.orgStride; L.cs = j.curStride;
        L.w = w; L.kind = kind; L.cmax = ( 1 << j.bitDepth ) - 1;
        L.wt = j.wp.w; L.off = j.wp.offset; L.sh = j.wp.shift; L.rnd = j.wp.round;
        L.maxDist = kind == VTMHIP_DIST_SAD ? j.maxDist : ~0ull;
        const bool def = j.wp.w == 1 << j.wp.shift, bi = j.isBiPred != 0;
        if( kind == VTMHIP_DIST_SAD ) L.mode = def ? ( j.wp.offset == 0 ? WPM_PLAIN : bi ? WPM_ADD : WPM_ADD_CLIP ) : bi ? WPM_PEL : WPM_CLIP;
        else if( kind == VTMHIP_DIST_SSE ) L.mode = bi ? WPM_PEL : WPM_CLIP;
        else L.mode = WPM_PEL;
        if( kind == VTMHIP_DIST_SATD )
        {
          L.tile = ( ( w | h ) & 7 ) == 0 ? 8 : ( ( w | h ) & 3 ) == 0 ? 4 : 2;
          L.tpr = FastDiv( w / L.tile );
          items = ( h / L.tile ) * L.tpr.d;
        }
        else items = h;
      }
      else out[g.job] = VTMHIP_WP_INVALID_DIST;
    }
    const int total = wave_scan_items( lane, items, sEnd[wv] );
    __syncthreads();

    // the wave walks the group's items 64 at a time; lane's item t = b + lane: its job index only grows
    WaveCursor         cur;
    WpJobL             L {};
    int                carryJob = -1;   // the job of lane 63 in the previous step and its prefix there
    unsigned long long carrySum = 0;
    for( int b = 0; b < total; b += 64 )   // wave-uniform: the shuffles below see every lane
    {
      const int          t   = b + lane;
      const bool         act = t < total;
      int                key = -1;
      unsigned long long v   = 0;
      if( act )
      {
        if( cur.beyond( t ) ) { cur.advance( t, sEnd[wv] ); L = sJob[wv][cur.cj]; }
        v   = wp_item( L, t - cur.start );
        key = cur.cj;
      }
      // segmented inclusive scan: the items of one job are consecutive lanes
#pragma unroll
      for( int o = 1; o < 64; o <<= 1 )
      {
        const unsigned long long u = __shfl_up( v, o, 64 );
        const int                k = __shfl_up( key, o, 64 );
        if( lane >= o && k == key ) v += u;
      }
      const unsigned long long prefix = v + ( act && key == carryJob ? carrySum : 0ull );
      unsigned long long       prev   = __shfl_up( prefix, 1, 64 );   // the prefix before this item's row / tile
      const int                pk     = __shfl_up( key, 1, 64 );
      if( lane == 0 || pk != key ) prev = key == carryJob ? carrySum : 0ull;
      if( act )
      {
        const bool over = L.maxDist < prefix, wasOver = L.maxDist < prev;   // SADw: `if( maximumDistortionForEarlyExit < uiSum ) return uiSum` per row
        if( ( over && !wasOver ) || ( !over && t == cur.end - 1 ) ) out[g.base + cur.cj] = prefix;
      }
      carryJob = __shfl( key, 63, 64 );
      carrySum = __shfl( prefix, 63, 64 );
    }
    __syncthreads();   // sJob / sEnd are rewritten by the next round
  }
}

int wp_dist_launch( vtmhip_ctx *ctx, const int16_t *d_orgBase, const int16_t *d_curBase, const vtmhip_wp_dist_job *d_jobs, int n, int G, unsigned long long *d_out )
{
  const int blocks = wave_blocks( n, G, WP_WAVES, ctx->numCUs * 64 );
  VTMHIP_TIME_KERNEL( ctx, "wp_dist_kernel" );
  hipLaunchKernelGGL( wp_dist_kernel, dim3( blocks ), dim3( 64 * WP_WAVES ), 0, ctx->stream, d_orgBase, d_curBase, d_jobs, n, G, d_out );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

// addWeightUni / addWeightBi of one job per wave
__global__ __launch_bounds__( 256 ) void wp_pred_kernel( const int16_t *__restrict__ src0Base, const int16_t *__restrict__ src1Base, int16_t *__restrict__ dstBase,
                                                        const vtmhip_wp_pred_job *__restrict__ jobs, int n )
{
  const int job = blockIdx.x * 4 + ( threadIdx.x >> 6 ), lane = threadIdx.x & 63;
  if( job >= n ) return;
  const vtmhip_wp_pred_job j = jobs[job];
  if( !wp_pred_ok( j ) ) return;
  const int      shiftNum = max( 2, 14 - ( int ) j.bitDepth );   // IF_INTERNAL_FRAC_BITS( clpRng.bd ) (InterpolationFilter.h:54)
  const int      cmax     = ( 1 << j.bitDepth ) - 1, w = j.width, segs = ( w + 3 ) >> 2;
  const bool     bi       = j.mode == VTMHIP_WP_BI;
  // uni with the default weight (w0 == 1 << shift): noWeightUnidir / noWeightOffsetUnidir, i.e. weight 1 and shift shiftNum (an offset of 0 adds nothing)
  const bool     def      = !bi && j.w0 == 1 << j.shift;
  const int      s        = def ? shiftNum : j.shift + shiftNum;
  const int      w0       = def ? 1 : j.w0, w1 = j.w1;
  const int      rnd      = 1 << ( s - 1 );                       // s >= 2; bi: bRoundLuma = true
  const int      biAdd    = rnd + j.offset * ( 1 << ( s - 1 ) );   // weightBidir: round + (offset << (shift - 1))
  const int16_t *p0 = src0Base + j.src0Off, *p1 = src1Base + j.src1Off;
  int16_t       *d  = dstBase + j.dstOff;
  for( int i = lane; i < j.height * segs; i += 64 )
  {
    const int y = i / segs, x0 = ( i - y * segs ) << 2;
#pragma unroll
    for( int k = 0; k < 4; k++ )
    {
      const int x = x0 + k;
      if( x >= w ) break;
      const int a = p0[( long ) y * j.src0Stride + x] + 8192;   // P + IF_INTERNAL_OFFS
      int       v;
      if( bi ) v = ( w0 * a + w1 * ( p1[( long ) y * j.src1Stride + x] + 8192 ) + biAdd ) >> s;   // weightBidir
      else v = ( ( w0 * a + rnd ) >> s ) + j.offset;                                              // weightUnidir / noWeight(Offset)Unidir
      d[( long ) y * j.dstStride + x] = ( int16_t ) min( max( v, 0 ), cmax );
    }
  }
}

int wp_single( vtmhip_ctx *ctx, int kind, const int16_t *org, int orgStride, const int16_t *cur, int curStride, int width, int height, const vtmhip_wp_param *wp,
               int bitDepth, int isBiPred, uint64_t maxDist, uint64_t *dist )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, org && cur && wp && dist, "null pointer" );
  VTMHIP_REQUIRE( ctx, wp_dist_ok( width, height, kind, bitDepth, isBiPred, *wp ),
                  "outside the weighted-prediction sample contract (width / height 1..128, bitDepth 8..12, isBiPred 0 / 1, w in [-256, 256], shift 0..8, "
                  "offset / round in int16, even width and height on the 2x2 HAD path)" );
  // stage org and cur compactly (stride = width), then the job and the result slot
  HostStage    s( ctx );
  const size_t blk = ( size_t ) width * height * sizeof( int16_t );
  const size_t orgOff = s.region( blk ), curOff = s.region( blk ), jobOff = s.region( sizeof( vtmhip_wp_dist_job ) ), outOff = s.region( 8 );
  VTMHIP_TRY( s.reserve() );
  s.pack( orgOff, org, orgStride, width, height );
  s.pack( curOff, cur, curStride, width, height );
  vtmhip_wp_dist_job j;
  memset( &j, 0, sizeof( j ) );
  j.orgOff = ( int64_t ) ( orgOff / 2 ); j.curOff = ( int64_t ) ( curOff / 2 ); j.orgStride = width; j.curStride = width;
  j.width = ( int16_t ) width; j.height = ( int16_t ) height; j.kind = ( uint8_t ) kind; j.bitDepth = ( uint8_t ) bitDepth; j.isBiPred = ( uint8_t ) isBiPred;
  j.wp = *wp; j.maxDist = maxDist;
  s.put( jobOff, j );
  VTMHIP_TRY( s.upload( 0, outOff ) );
  VTMHIP_TRY( wp_dist_launch( ctx, s.dev<const int16_t>( 0 ), s.dev<const int16_t>( 0 ), s.dev<const vtmhip_wp_dist_job>( jobOff ), 1, 1, s.dev<unsigned long long>( outOff ) ) );
  VTMHIP_TRY( s.fetch( outOff, 8 ) );
  memcpy( dist, s.hp + outOff, 8 );
  return VTMHIP_OK;
}

}   // namespace

extern "C"
{

int vtmhip_xGetSADw( vtmhip_ctx *ctx, const int16_t *org, int orgStride, const int16_t *cur, int curStride, int width, int height, const vtmhip_wp_param *wp,
                     int bitDepth, int isBiPred, uint64_t maxDist, uint64_t *dist )
{
  return wp_single( ctx, VTMHIP_DIST_SAD, org, orgStride, cur, curStride, width, height, wp, bitDepth, isBiPred, maxDist, dist );
}

int vtmhip_xGetSSEw( vtmhip_ctx *ctx, const int16_t *org, int orgStride, const int16_t *cur, int curStride, int width, int height, const vtmhip_wp_param *wp,
                     int bitDepth, int isBiPred, uint64_t *dist )
{
  return wp_single( ctx, VTMHIP_DIST_SSE, org, orgStride, cur, curStride, width, height, wp, bitDepth, isBiPred, UINT64_MAX, dist );
}

int vtmhip_xGetHADsw( vtmhip_ctx *ctx, const int16_t *org, int orgStride, const int16_t *cur, int curStride, int width, int height, const vtmhip_wp_param *wp,
                      int bitDepth, int isBiPred, uint64_t *dist )
{
  return wp_single( ctx, VTMHIP_DIST_SATD, org, orgStride, cur, curStride, width, height, wp, bitDepth, isBiPred, UINT64_MAX, dist );
}

int vtmhip_wp_dist_batch_dev( vtmhip_ctx *ctx, const int16_t *d_orgBase, const int16_t *d_curBase, const vtmhip_wp_dist_job *d_jobs, int n, uint64_t *d_dist )
{
  VTMHIP_BATCH_ENTRY( ctx, n, d_orgBase && d_curBase && d_jobs && d_dist );
  return wp_dist_launch( ctx, d_orgBase, d_curBase, d_jobs, n, wave_jobs_per_wave( ctx->numCUs, n ), ( unsigned long long * ) d_dist );
}

int vtmhip_wp_pred_batch_dev( vtmhip_ctx *ctx, const int16_t *d_src0Base, const int16_t *d_src1Base, int16_t *d_dstBase, const vtmhip_wp_pred_job *d_jobs, int n )
{
  VTMHIP_BATCH_ENTRY( ctx, n, d_src0Base && d_src1Base && d_dstBase && d_jobs );
  VTMHIP_TIME_KERNEL( ctx, "wp_pred_kernel" );
  hipLaunchKernelGGL( wp_pred_kernel, dim3( ( n + 3 ) / 4 ), dim3( 256 ), 0, ctx->stream, d_src0Base, d_src1Base, d_dstBase, d_jobs, n );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

}   // extern "C"
