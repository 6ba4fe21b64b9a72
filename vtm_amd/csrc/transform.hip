// transform.hip -- separable DCT-2 / DST-7 / DCT-8 (2..64 points), scalar quantisation / dequantisation.
//
// Reference: CommonLib/TrQuant.cpp xT :776-851, xIT :853-923, tables fastFwdTrans/fastInvTrans :69-81;
// CommonLib/TrQuant_EMT.cpp (the "fast" butterflies are exact refactorings of the matrix product
// _fastForwardMM :274-323 / _fastInverseMM :235-271 -- no intermediate rounding -- so a plain 32-bit integer
// matrix product is bit-identical, wrap-around included); core matrices CommonLib/RomTr.cpp (H.266 8.7.4.2
// transMatrix constants, regenerated procedurally in tr_tables.hpp); Quant::quant CommonLib/Quant.cpp:955-1038,
// Quant::dequant :357-482 (flat scaling list), scales CommonLib/Rom.cpp:463-473.
//
// One workgroup per transform unit.  The residual block, the intermediate (transposed) block and the transposed core
// matrix live in LDS; lane l of a wave produces output frequency k = l (matrix columns are contiguous in LDS, the data
// row is a broadcast), so LDS reads are conflict-free.
#include "ctx.hpp"
#include "stage.hpp"
#include "bucket.hpp"
#include "tr_tables.hpp"
#include "lmcs.hpp"
#include "tu_stages.hpp"

#include <cmath>
#include <vector>

// The core matrices live in the CONTEXT (one copy per context, on the context's device, freed by vtmhip_destroy): no process-global
// state, so two contexts on two GPUs -- or two encoder threads with a context each -- cannot race or see the other device's pointers.
int vtmhip_internal_tr_tables( vtmhip_ctx *ctx )
{
  std::lock_guard<std::mutex> lock( ctx->initMutex );
  if( ctx->trTabBuf ) return VTMHIP_OK;
  VTMHIP_HIP( ctx, hipSetDevice( ctx->device ) );
  std::vector<int16_t> host;
  size_t               offs[3][7];
  for( int t = 0; t < 3; t++ )
    for( int l = 0; l < 7; l++ )
    {
      offs[t][l] = ( size_t ) -1;
      const int n = 1 << l;
      std::vector<int16_t> m( ( size_t ) n * n );
      if( n >= 2 && vtmhip_tr_matrix( t, n, m.data() ) == 0 )
      {
        offs[t][l] = host.size();
        host.insert( host.end(), m.begin(), m.end() );
      }
    }
  int16_t *dbuf = nullptr;
  VTMHIP_HIP( ctx, hipMalloc( ( void ** ) &dbuf, host.size() * sizeof( int16_t ) ) );
  if( hipMemcpy( dbuf, host.data(), host.size() * sizeof( int16_t ), hipMemcpyHostToDevice ) != hipSuccess )
  {
    ( void ) hipFree( dbuf );
    ctx->lastError = "hipMemcpy of the transform core matrices failed";
    return VTMHIP_E_HIP;
  }
  for( int t = 0; t < 3; t++ )
    for( int l = 0; l < 7; l++ ) ctx->trTab[t][l] = offs[t][l] == ( size_t ) -1 ? nullptr : dbuf + offs[t][l];
  ctx->trTabBuf = dbuf;
  return VTMHIP_OK;
}

namespace
{

struct TrTables { const int16_t *m[3][7]; };   // [type][log2 N] -> device pointer to the N x N forward matrix (row-major)

TrTables tabs_of( const vtmhip_ctx *ctx )
{
  TrTables t;
  for( int a = 0; a < 3; a++ )
    for( int l = 0; l < 7; l++ ) t.m[a][l] = ctx->trTab[a][l];
  return t;
}

constexpr int TB = 64;   // MAX_TB_SIZEY

__global__ __launch_bounds__( 256 ) void xT_kernel( const int16_t *__restrict__ resiBase, int *__restrict__ coefBase,
                                                   const vtmhip_tr_job *__restrict__ jobs, TrTables tabs, int *__restrict__ sumAbsOut )
{
  extern __shared__ __attribute__( ( aligned( 16 ) ) ) int ldsw[];
  const vtmhip_tr_job j = jobs[blockIdx.x];
  const int           w = j.width, h = j.height, bd = j.bitDepth;
  int                *blk = ldsw;                    // [h][w]
  int                *tmp = blk + w * h;             // [w][h+1]
  int16_t            *sMT = ( int16_t * ) ( tmp + w * ( h + 1 ) );
  const int16_t      *resi = resiBase + j.srcOff;
  int                *coef = coefBase + j.dstOff;
  const int           t = threadIdx.x, step = blockDim.x;
  for( int i = t; i < w * h; i += step )
  {
    const int y = i / w, x = i - y * w;
    blk[i]      = resi[( long ) y * j.srcStride + x];
  }
  const int skipW = tr_skip( j.typeHor, w ), skipH = tr_skip( j.typeVer, h );
  int       sumAbs = 0;
  if( w > 1 && h > 1 )
  {
    lds_load_matrix_T( tabs.m[j.typeHor][ilog2( w )], w, sMT, t, step );
    __syncthreads();
    lds_fwd_pass( blk, w, tmp, h + 1, sMT, w, h, ALL_LINES, w - skipW, ilog2( w ) + bd + 6 - 15, t, step, ( int * ) nullptr );   // tmp[k][y]
    __syncthreads();
    lds_load_matrix_T( tabs.m[j.typeVer][ilog2( h )], h, sMT, t, step );
    __syncthreads();
    // second pass straight to global: coef[k2 * w + j2], zero where j2 >= w - skipW or k2 >= h - skipH
    lds_fwd_pass( tmp, h + 1, coef, w, sMT, h, w, w - skipW, h - skipH, ilog2( h ) + 6, t, step, &sumAbs );
  }
  else
  {
    // 1-D cases (W == 1 or H == 1, TrQuant.cpp:836-850)
    const int n = h == 1 ? w : h, type = h == 1 ? j.typeHor : j.typeVer, skip = h == 1 ? skipW : skipH;
    lds_load_matrix_T( tabs.m[type][ilog2( n )], n, sMT, t, step );
    __syncthreads();
    lds_fwd_pass( blk, n, coef, 1, sMT, n, 1, ALL_LINES, n - skip, ilog2( n ) + bd + 6 - 15, t, step, &sumAbs );
  }
  if( sumAbsOut )
  {
    // sum |coef| of the block (MTS candidate pre-selection, TrQuant.cpp:986-990); block-wide reduction through LDS
    __syncthreads();
    sumAbs = wave_reduce_add( sumAbs );
    if( ( threadIdx.x & 63 ) == 0 ) blk[threadIdx.x >> 6] = sumAbs;
    __syncthreads();
    if( threadIdx.x == 0 )
    {
      int s = 0;
      for( int k = 0; k < ( int ) ( blockDim.x >> 6 ); k++ ) s += blk[k];
      sumAbsOut[blockIdx.x] = s;
    }
  }
}

__global__ __launch_bounds__( 256 ) void xIT_kernel( const int *__restrict__ coefBase, int16_t *__restrict__ resiBase,
                                                    const vtmhip_tr_job *__restrict__ jobs, TrTables tabs )
{
  extern __shared__ __attribute__( ( aligned( 16 ) ) ) int ldsw[];
  const vtmhip_tr_job j = jobs[blockIdx.x];
  const int           w = j.width, h = j.height, bd = j.bitDepth;
  int                *blk = ldsw;                  // coefficients [h][w]
  int                *tmp = blk + w * h;           // [w][h]
  int16_t            *sM  = ( int16_t * ) ( tmp + w * h );
  const int          *coef = coefBase + j.srcOff;
  int16_t            *resi = resiBase + j.dstOff;
  const int           t = threadIdx.x, step = blockDim.x;
  for( int i = t; i < w * h; i += step ) blk[i] = coef[i];
  const int skipW = tr_skip( j.typeHor, w ), skipH = tr_skip( j.typeVer, h );
  if( w > 1 && h > 1 )
  {
    lds_load_matrix( tabs.m[j.typeVer][ilog2( h )], h, sM, t, step );
    __syncthreads();
    lds_inv_pass( blk, w, sM, h, w, w - skipW, h - skipH, 7, t, step, [&]( int, int i, int y, int v ) { tmp[i * h + y] = v; } );   // tmp[i (x-frequency)][y]
    __syncthreads();
    lds_load_matrix( tabs.m[j.typeHor][ilog2( w )], w, sM, t, step );
    __syncthreads();
    lds_inv_pass( tmp, h, sM, w, h, ALL_LINES, w - skipW, 20 - bd, t, step, [&]( int, int y, int x, int v ) { resi[( long ) y * j.dstStride + x] = ( int16_t ) v; } );
  }
  else
  {
    const int n = w == 1 ? h : w, type = w == 1 ? j.typeVer : j.typeHor, skip = w == 1 ? skipH : skipW;
    lds_load_matrix( tabs.m[type][ilog2( n )], n, sM, t, step );
    __syncthreads();
    lds_inv_pass( blk, 1, sM, n, 1, ALL_LINES, n - skip, 20 - bd + 1, t, step, [&]( int, int, int i, int v ) { resi[w == 1 ? ( long ) i * j.dstStride : i] = ( int16_t ) v; } );
  }
}

// 1-D pointer-surface kernels (FwdTrans / InvTrans signatures, arbitrary int32 input)
__global__ __launch_bounds__( 256 ) void fwd1d_kernel( const int *__restrict__ src, int *__restrict__ dst, const int16_t *__restrict__ m, int N, int shift,
                                                      int line, int skip1, int skip2 )
{
  const int      rl = line - skip1, cut = N - skip2;
  const unsigned rnd = shift > 0 ? 1u << ( shift - 1 ) : 0;
  for( int o = blockIdx.x * blockDim.x + threadIdx.x; o < N * line; o += gridDim.x * blockDim.x )
  {
    const int k = o / line, j = o - k * line;
    int       v = 0;
    if( j < rl && k < cut )
    {
      unsigned sum = 0;
      for( int n = 0; n < N; n++ ) sum += ( unsigned ) src[j * N + n] * ( unsigned ) ( int ) m[k * N + n];
      v = ( int ) ( sum + rnd ) >> shift;
    }
    dst[o] = v;
  }
}

__global__ __launch_bounds__( 256 ) void inv1d_kernel( const int *__restrict__ src, int *__restrict__ dst, const int16_t *__restrict__ m, int N, int shift,
                                                      int line, int skip1, int skip2, int cmin, int cmax )
{
  const int      rl = line - skip1, cut = N - skip2;
  const unsigned rnd = 1u << ( shift - 1 );
  for( int o = blockIdx.x * blockDim.x + threadIdx.x; o < N * line; o += gridDim.x * blockDim.x )
  {
    const int i = o / N, jj = o - i * N;
    int       v = 0;
    if( i < rl )
    {
      unsigned sum = 0;
      for( int k = 0; k < cut; k++ ) sum += ( unsigned ) src[k * line + i] * ( unsigned ) ( int ) m[k * N + jj];
      v = min( cmax, max( cmin, ( int ) ( sum + rnd ) >> shift ) );
    }
    dst[o] = v;
  }
}

// ---- scalar quantisation (flat scaling list): tu_stages.hpp's QuantRule per job -------------------------------------------
__device__ __forceinline__ QuantRule quant_rule_of( const vtmhip_quant_job &j )
{
  return quant_rule( j.bitDepth, j.qpPer, j.qpRem, j.isIRAP, ilog2( j.width ), ilog2( j.height ), j.isTransformSkip );
}

__global__ __launch_bounds__( 256 ) void quant_kernel( const int *__restrict__ coefBase, int *__restrict__ qBase, int *__restrict__ deltaUBase,
                                                      const vtmhip_quant_job *__restrict__ jobs, int *__restrict__ absSumOut )
{
  __shared__ int            sRed[4];
  const vtmhip_quant_job j  = jobs[blockIdx.x];
  const int              w = j.width, h = j.height;
  const QuantRule        qr = quant_rule_of( j );
  const int             *coef = coefBase + j.srcOff;
  int                   *q    = qBase + j.dstOff;
  int                    sum  = 0;
  for( int i = threadIdx.x; i < w * h; i += blockDim.x )
  {
    // the reference's scan covers only the 32x32 zero-out region of larger blocks: positions outside keep level 0 (Quant.cpp:1004-1008)
    if( ( i % w ) >= 32 || ( i / w ) >= 32 ) { q[i] = 0; if( deltaUBase ) deltaUBase[j.dstOff + i] = 0; continue; }
    const int c = coef[i];
    long long t;
    const int mag = qr.mag( c, t );
    if( deltaUBase ) deltaUBase[j.dstOff + i] = ( int ) ( ( t - ( ( long long ) mag << qr.qBits ) ) >> ( qr.qBits - 8 ) );
    sum += mag;
    q[i] = qr.signed_level( c, mag );
  }
  sum = wave_reduce_add( sum );
  if( ( threadIdx.x & 63 ) == 0 ) sRed[threadIdx.x >> 6] = sum;
  __syncthreads();
  if( threadIdx.x == 0 ) absSumOut[blockIdx.x] = sRed[0] + sRed[1] + sRed[2] + sRed[3];
}

__global__ __launch_bounds__( 256 ) void dequant_kernel( const int *__restrict__ qBase, int *__restrict__ coefBase,
                                                        const vtmhip_quant_job *__restrict__ jobs )
{
  const vtmhip_quant_job j = jobs[blockIdx.x];
  const QuantRule        qr = quant_rule_of( j );   // the dequant half
  const int             *q    = qBase + j.srcOff;
  int                   *coef = coefBase + j.dstOff;
  for( int i = threadIdx.x; i < j.width * j.height; i += blockDim.x ) coef[i] = qr.dequant( q[i] );
}


// ---- fused residual-coding chain of one TU: xT -> Quant::quant -> Quant::dequant -> xIT -> SSE(residual, reconstructed residual) ----
// = transformNxN + invTransformNxN + getDistPart( DF_SSE ) of xEstimateInterResidualQT (EncoderLib/InterSearch.cpp:6637-6733) without the
// CABAC bit estimate in between (host).  The stages are tu_stages.hpp's.  Everything stays in LDS; TPT threads per TU (64: four independent TUs
// per workgroup, wave-level synchronisation only; 256: one TU per workgroup).
//
// CRS (the three chain kernels): LMCS chroma residual scaling fused in (vtmhip_tu_chain_crs_batch_dev; reference InterSearch.cpp:6628-6632, 6728-6733) -- two
// per-sample hooks with lmcs.hpp's rules: at the load the working block gets fwd( r ) while the SSE copy keeps r, and in the epilogue the reconstruction goes
// through inv() before the rec store and the SSE.  The job's adj (vtmhip_tu_job.chromaAdj) is 0 for "leave this job alone".  CRS == false is the plain chain.
__device__ __forceinline__ QuantRule quant_rule_of( const vtmhip_tu_job &j, int lw, int lh, bool ts ) { return quant_rule( j.bitDepth, j.qpPer, j.qpRem, j.isIRAP, lw, lh, ts ); }

__device__ __forceinline__ void sse_add( long long &sse, int d ) { sse += ( long long ) ( unsigned long long ) ( ( unsigned ) d * ( unsigned ) d ); }

// the packing of the three reduced sums { sumAbs, absSum, sse }
struct TuResultStore
{
  vtmhip_tu_result *out;
  __device__ __forceinline__ void operator()( const long long ( &v )[3] ) const
  {
    vtmhip_tu_result r;
    r.sse = ( uint64_t ) v[2]; r.sumAbs = ( int32_t ) v[0]; r.absSum = ( int32_t ) v[1];
    *out = r;
  }
};

// What the chain kernels may leave out (the `flags` argument; on unless the environment says otherwise):
//   TU_ZERO_SKIP   VTMHIP_TU_ZERO_SKIP=0    the inverse half runs for TUs without a non-zero level too
enum { TU_ZERO_SKIP = 1 };

static int tu_chain_flags()
{
  static const int flags = env_switch( "VTMHIP_TU_ZERO_SKIP", true ) ? TU_ZERO_SKIP : 0;
  return flags;
}

template<int TPT, bool CRS>
__global__ __launch_bounds__( 256 ) void tu_chain_kernel( const int16_t *__restrict__ resiBase, const vtmhip_tu_job *__restrict__ jobs, int numJobs,
                                                         TrTables tabs, int *__restrict__ levelsBase, int16_t *__restrict__ recBase,
                                                         vtmhip_tu_result *__restrict__ results, int maxW, int maxH, int flags )
{
  extern __shared__ __attribute__( ( aligned( 16 ) ) ) int ldsw[];
  __shared__ long long sRed[4][3];
  constexpr int TUS = 256 / TPT;
  const int     sub = TPT == 64 ? ( int ) ( threadIdx.x >> 6 ) : 0, t = TPT == 64 ? ( int ) ( threadIdx.x & 63 ) : ( int ) threadIdx.x;
  const int     jobIdx = blockIdx.x * TUS + sub;
  if( jobIdx >= numJobs ) return;   // TPT == 64: whole waves leave; TPT == 256: grid == numJobs
  const vtmhip_tu_job j = jobs[jobIdx];
  const int           w = j.width, h = j.height, bd = j.bitDepth;
  const int           mx = maxW > maxH ? maxW : maxH;
  const int           perTu = maxW * maxH + maxW * ( maxH + 1 ) + ( ( mx * mx + 1 ) >> 1 ) + ( ( maxW * maxH + 1 ) >> 1 );   // ints
  int                *blk = ldsw + sub * perTu;            // [h][w] residual -> coefficients -> dequantised coefficients
  int                *tmp = blk + maxW * maxH;             // [w][h+1] / [w][h]
  int16_t            *sM  = ( int16_t * ) ( tmp + maxW * ( maxH + 1 ) );
  int16_t            *sR  = sM + ( ( mx * mx + 1 ) & ~1 );   // residual copy for the SSE
  const int16_t      *resi = resiBase + j.resiOff;
  const int           adj = CRS ? lmcs_job_adj( j.chromaAdj, w, h ) : 0, maxAbs = ( 1 << bd ) - 1;
  const LmcsScale     sc  = lmcs_scale_of( CRS && adj ? adj : 1 );
  for( int i = t; i < w * h; i += TPT )
  {
    const int y = i / w, x = i - y * w;
    const int16_t v = resi[( long ) y * j.resiStride + x];
    blk[i] = CRS && adj ? lmcs_fwd( v, sc, maxAbs ) : v;
    sR[i]  = v;
  }
  const int lw = ilog2( w ), lh = ilog2( h );
  long long sumAbs = 0, absSum = 0, sse = 0;
  const bool ts = j.typeHor == VTMHIP_TRSKIP;   // MTS_SKIP candidate: the coefficients are the residual samples
  const int  skipW = ts ? 0 : tr_skip( j.typeHor, w ), skipH = ts ? 0 : tr_skip( j.typeVer, h );
  chain_sync<TPT>();
  if( ts )
  {
    const QuantRule qr = quant_rule_of( j, lw, lh, true );
    int            *levels = levelsBase ? levelsBase + j.outOff : nullptr;
    int16_t        *rec    = recBase ? recBase + j.outOff : nullptr;
    for( int i = t; i < w * h; i += TPT )
    {
      const int c = blk[i];
      sumAbs += abs( c );
      const int q = qr.level( c, absSum );
      if( levels ) levels[i] = q;
      int v = ( int ) ( int16_t ) qr.dequant( q );
      if( CRS && adj ) v = lmcs_inv( v, adj, maxAbs );
      if( rec ) rec[i] = ( int16_t ) v;
      sse_add( sse, ( CRS ? ( int ) sR[i] : c ) - v );   // CRS: c is the scaled sample, the distortion is taken against the kept copy
    }
  }
  else
  {
    // forward: TrQuant::xT
    lds_load_matrix_T( tabs.m[j.typeHor][lw], w, sM, t, TPT );
    chain_sync<TPT>();
    lds_fwd_pass( blk, w, tmp, h + 1, sM, w, h, ALL_LINES, w - skipW, lw + bd + 6 - 15, t, TPT, ( long long * ) nullptr );
    chain_sync<TPT>();
    lds_load_matrix_T( tabs.m[j.typeVer][lh], h, sM, t, TPT );
    chain_sync<TPT>();
    lds_fwd_pass( tmp, h + 1, blk, w, sM, h, w, w - skipW, h - skipH, lh + 6, t, TPT, &sumAbs );
    chain_sync<TPT>();
    // Quant::quant + Quant::dequant, in place
    {
      const QuantRule qr = quant_rule_of( j, lw, lh, false );
      int            *levels = levelsBase ? levelsBase + j.outOff : nullptr;
      for( int i = t; i < w * h; i += TPT )
      {
        const int q = qr.level( blk[i], absSum );
        if( levels ) levels[i] = q;
        blk[i] = qr.dequant( q );
      }
    }
    int16_t *rec = recBase ? recBase + j.outOff : nullptr;
    if( chain_sync_none<TPT>( absSum != 0 ) && ( flags & TU_ZERO_SKIP ) )
    {
      // no non-zero level (this wave's TU / this workgroup's): the inverse of zeros is zero, see tu_chain_uni_kernel
      for( int i = t; i < w * h; i += TPT )
      {
        if( rec ) rec[i] = 0;
        sse_add( sse, ( int ) sR[i] );
      }
    }
    else
    {
      // inverse: TrQuant::xIT, then SSE against the residual
      lds_load_matrix( tabs.m[j.typeVer][lh], h, sM, t, TPT );
      chain_sync<TPT>();
      lds_inv_pass( blk, w, sM, h, w, w - skipW, h - skipH, 7, t, TPT, [&]( int, int i, int y, int v ) { tmp[i * h + y] = v; } );
      chain_sync<TPT>();
      lds_load_matrix( tabs.m[j.typeHor][lw], w, sM, t, TPT );
      chain_sync<TPT>();
      lds_inv_pass( tmp, h, sM, w, h, ALL_LINES, w - skipW, 20 - bd, t, TPT, [&]( int o, int, int, int v ) {
        if( CRS && adj ) v = lmcs_inv( v, adj, maxAbs );
        if( rec ) rec[o] = ( int16_t ) v;
        sse_add( sse, ( int ) sR[o] - ( int ) ( int16_t ) v );
      } );
    }
  }
  long long sums[3] = { sumAbs, absSum, sse };
  chain_reduce_store<TPT, 3>( sums, sRed, sub, t, true, TuResultStore{ results + jobIdx } );
}


// ---- the smallest TUs (4x4, 8x4, 4x8: the chroma TUs of 8x8 / 16x8 / 8x16 PUs; 4x4 luma) of a uniform batch: ONE LANE per TU ---------------------------
// The whole block lives in registers (W * H <= 32 values), the 4- / 8-point core matrices of the three types sit in LDS (staged once per workgroup);
// the generic kernel above spends 64 threads and a dozen LDS round trips on such a block.  Same arithmetic, same order of the integer operations.
template<int W, int H, bool CRS>
__global__ __launch_bounds__( 256 ) void tu_chain_lane_kernel( const int16_t *__restrict__ resiBase, const vtmhip_tu_job *__restrict__ jobs, int numJobs, TrTables tabs,
                                                              int *__restrict__ levelsBase, int16_t *__restrict__ recBase, vtmhip_tu_result *__restrict__ results )
{
  constexpr int LW = W == 4 ? 2 : 3, LH = H == 4 ? 2 : 3, N = W * H;
  __shared__ int16_t sMH[3][W * W], sMV[3][H * H];
  for( int i = threadIdx.x; i < 3 * W * W; i += 256 ) sMH[i / ( W * W )][i % ( W * W )] = tabs.m[i / ( W * W )][LW][i % ( W * W )];
  for( int i = threadIdx.x; i < 3 * H * H; i += 256 ) sMV[i / ( H * H )][i % ( H * H )] = tabs.m[i / ( H * H )][LH][i % ( H * H )];
  __syncthreads();
  const int jobIdx = blockIdx.x * 256 + threadIdx.x;
  if( jobIdx >= numJobs ) return;
  const vtmhip_tu_job j = jobs[jobIdx];
  if( j.width != W || j.height != H || j.typeHor > 2 || j.typeVer > 2 ) return;   // the caller's promise is broken: leave the result untouched
  const int      bd = j.bitDepth;
  const int16_t *mh = sMH[j.typeHor], *mv = sMV[j.typeVer];
  int            r[N], b[N];
  const int16_t *resi = resiBase + j.resiOff;
  if( ( ( j.resiOff | j.resiStride ) & 3 ) == 0 )   // 8-byte aligned rows (offsets and strides of 4-sample blocks normally are): 4 samples per load
  {
#pragma unroll
    for( int y = 0; y < H; y++ )
#pragma unroll
      for( int x = 0; x < W; x += 4 )
      {
        const int2 v = *reinterpret_cast<const int2 *>( resi + ( long ) y * j.resiStride + x );
        r[y * W + x] = ( int ) ( short ) v.x; r[y * W + x + 1] = v.x >> 16; r[y * W + x + 2] = ( int ) ( short ) v.y; r[y * W + x + 3] = v.y >> 16;
      }
  }
  else
  {
#pragma unroll
    for( int y = 0; y < H; y++ )
#pragma unroll
      for( int x = 0; x < W; x++ ) r[y * W + x] = resi[( long ) y * j.resiStride + x];
  }
  // CRS: r becomes fwd( r ); the epilogue reads the unscaled residual again (L2) instead of holding a second block in registers
  const int adj = CRS ? lmcs_job_adj( j.chromaAdj, W, H ) : 0, maxAbs = ( 1 << bd ) - 1;
  if( CRS && adj )
  {
    const LmcsScale sc = lmcs_scale_of( adj );
#pragma unroll
    for( int i = 0; i < N; i++ ) r[i] = lmcs_fwd( r[i], sc, maxAbs );
  }
  long long sumAbs = 0, absSum = 0, sse = 0;
  lane_fwd_2d<W, H>( r, b, mh, mv, bd, sumAbs );
  // Quant::quant + Quant::dequant, flat scaling list
  {
    const QuantRule qr = quant_rule_of( j, LW, LH, false );
    int            *levels = levelsBase ? levelsBase + j.outOff : nullptr;
#pragma unroll
    for( int i = 0; i < N; i++ )
    {
      const int q = qr.level( b[i], absSum );
      if( levels ) levels[i] = q;
      b[i] = qr.dequant( q );
    }
  }
  // inverse, SSE against the residual
  int16_t *rec = recBase ? recBase + j.outOff : nullptr;
  lane_inv_2d<W, H>( b, mh, mv, bd, [&]( int y, int x, int v ) {
    if( CRS && adj ) v = lmcs_inv( v, adj, maxAbs );
    if( rec ) rec[y * W + x] = ( int16_t ) v;
    sse_add( sse, ( CRS ? ( int ) resi[( long ) y * j.resiStride + x] : r[y * W + x] ) - v );
  } );
  vtmhip_tu_result res;
  res.sse = ( uint64_t ) sse; res.sumAbs = ( int32_t ) sumAbs; res.absSum = ( int32_t ) absSum;
  results[jobIdx] = res;
}

template<int W, int H, bool CRS>
int launch_tu_lane( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_tu_job *d_jobs, int n, int32_t *d_levelsBase, int16_t *d_recBase, vtmhip_tu_result *d_results,
                    const TrTables &tb )
{
  VTMHIP_TIME_KERNEL( ctx, "tu_chain_lane_kernel" );
  hipLaunchKernelGGL( ( tu_chain_lane_kernel<W, H, CRS> ), dim3( ( n + 255 ) / 256 ), dim3( 256 ), 0, ctx->stream, d_resiBase, d_jobs, n, tb, d_levelsBase, d_recBase, d_results );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}


// ---- register-blocked fast path of the fused chain for batches of ONE TU size (W, H >= 8) --------------------------------------
// tu_stages.hpp's blocked passes: a lane owns 2 x 8 outputs of a pass.  LPT lanes share one TU; 256 / LPT TUs per workgroup; the matrices
// of the three transform types are staged once per workgroup.
template<int LPT, bool CRS>
__global__ __launch_bounds__( 256 ) void tu_chain_uni_kernel( const int16_t *__restrict__ resiBase, const vtmhip_tu_job *__restrict__ jobs, int numJobs,
                                                             TrTables tabs, int *__restrict__ levelsBase, int16_t *__restrict__ recBase,
                                                             vtmhip_tu_result *__restrict__ results, int w, int h, int *__restrict__ fwdCoefBase, int flags )
{
  // fwdCoefBase != nullptr: forward transform only (TrQuant::xT): coefficients to fwdCoefBase + outOff, sum|coef| to results
  extern __shared__ __attribute__( ( aligned( 16 ) ) ) int ldsw[];
  __shared__ long long sRed[4][3];
  constexpr int TUS = 256 / LPT;
  const int     sub = threadIdx.x / LPT, t = threadIdx.x - sub * LPT;
  const int     perTu = w * h + w * ( h + 1 );   // ints: blk, tmp (the 16-bit residual copy lives in blk until the second forward pass overwrites it)
  int16_t      *sMat = ( int16_t * ) ( ldsw + TUS * perTu );              // [dim][type][orientation][N*N]
  const int     lw = ilog2( w ), lh = ilog2( h );
  const int     hBase = ( w > 32 ? 2 : 6 ) * w * w;   // only DCT-2 exists above 32: one matrix pair instead of three
  const bool    sq    = w == h;                       // square TUs: both height matrices ARE the width's slots (tuq_pass_il reads the interleaved transpose)
  for( int ty = 0; ty < 3; ty++ )
  {
    // [type][slot]: slot 0 = M (the inverse passes), slot 1 = M^T (the forward passes; the height's is plain: 32-bit input)
    const int16_t *mw = ( ty == 0 || w <= 32 ) ? tabs.m[ty][lw] : nullptr, *mh = ( ty == 0 || h <= 32 ) ? tabs.m[ty][lh] : nullptr;   // DST-7 / DCT-8 exist up to 32
    if( mw ) tuq_stage_matrix<false>( mw, w, lw, sMat + ( ty * 2 ) * w * w, sMat + ( ty * 2 + 1 ) * w * w );
    if( mh && !sq ) tuq_stage_matrix<true>( mh, h, lh, sMat + hBase + ( ty * 2 ) * h * h, sMat + hBase + ( ty * 2 + 1 ) * h * h );
  }
  __syncthreads();
  const int  jobIdx = blockIdx.x * TUS + sub;
  const bool live   = jobIdx < numJobs;   // LPT <= 64: dead groups are whole waves or idle lane groups that only meet at the barriers
  vtmhip_tu_job j;
  if( live ) j = jobs[jobIdx];
  else { j = jobs[numJobs - 1]; }
  const int      bd = j.bitDepth;
  int           *blk = ldsw + sub * perTu, *tmp = blk + w * h;
  int16_t       *sR  = ( int16_t * ) blk;
  const int16_t *mW = sMat + ( j.typeHor * 2 ) * w * w;
  const int16_t *mH0 = sq ? sMat + ( j.typeVer * 2 ) * w * w : sMat + hBase + ( j.typeVer * 2 ) * h * h;          // M_H, rows k, k+1 interleaved
  const int16_t *mH1 = sq ? sMat + ( j.typeVer * 2 + 1 ) * w * w : sMat + hBase + ( j.typeVer * 2 + 1 ) * h * h;   // M_H^T: pair-interleaved (square) / plain
  const int16_t *resi = resiBase + j.resiOff;
  const int       adj = CRS ? lmcs_job_adj( j.chromaAdj, w, h ) : 0, maxAbs = ( 1 << bd ) - 1;
  const LmcsScale sc  = lmcs_scale_of( CRS && adj ? adj : 1 );
  for( int i = t; i < w * h; i += LPT )
  {
    const int y = i >> lw, x = i & ( w - 1 );
    const int16_t v = resi[( long ) y * j.resiStride + x];
    sR[i] = CRS && adj ? ( int16_t ) lmcs_fwd( v, sc, maxAbs ) : v;   // fwd() clips to +-(2^bitDepth - 1): the packed first pass keeps its headroom
  }
  int16_t *dq16 = reinterpret_cast<int16_t *>( tmp );   // dequantised coefficients [k][k2] (after the second forward pass has consumed tmp)
  int16_t *t16  = reinterpret_cast<int16_t *>( blk );   // first inverse pass output [y][i] (after quantisation has consumed blk)
  int     *rec32 = tmp;                                  // reconstructed residual [y][x]
  const int skipW = tr_skip( j.typeHor, w ), skipH = tr_skip( j.typeVer, h );
  long long sumAbs = 0, absSum = 0, sse = 0;
  chain_sync<LPT>();
  // forward (TrQuant::xT): tmp[k][y] = sum_n blk[y][n] * MT_hor[n][k];  blk[k2][j2] = sum_n tmp[j2][n] * MT_ver[n][k2]
  tuq_pass16<LPT, false>( sR, w, reinterpret_cast<const unsigned *>( mW + w * w ), w, h, w, h, w - skipW, tmp, 1, h + 1, lw + bd + 6 - 15, t );
  chain_sync<LPT>();
  if( sq ) tuq_pass_il<LPT, false>( tmp, h + 1, 1, reinterpret_cast<const unsigned *>( mH1 ), h, w, h, w - skipW, h - skipH, blk, 1, w, lh + 6, t, &sumAbs );
  else tuq_pass<LPT, false>( tmp, h + 1, 1, mH1, h, h, w, h, w - skipW, h - skipH, blk, 1, w, lh + 6, t, &sumAbs );
  chain_sync<LPT>();
  if( fwdCoefBase )
  {
    if( live )
      for( int i = t; i < w * h; i += LPT ) fwdCoefBase[j.outOff + i] = blk[i];
  }
  else
  {
    // Quant::quant + Quant::dequant (flat scaling list)
    {
      const QuantRule qr = quant_rule_of( j, lw, lh, false );
      int            *levels = ( levelsBase && live ) ? levelsBase + j.outOff : nullptr;
      for( int i = t; i < w * h; i += LPT )
      {
        const int q = qr.level( blk[i], absSum );
        if( levels ) levels[i] = q;
        dq16[( ( i & ( w - 1 ) ) << lh ) + ( i >> lw )] = ( int16_t ) qr.dequant( q );   // transposed: the vertical index contiguous
      }
    }
    // (The transposed dq16 stores above are wasted on the path below: the vote can only follow the loop that forms the levels.)
    // No non-zero level in this wave / workgroup (the reference's `if( currAbsSum > 0 )` around invTransformNxN, InterSearch.cpp:6693): the inverse of zeros is
    // zero -- (0 + rnd) >> shift = 0, clip( 0 ) = 0, lmcs_inv( 0 ) = 0 -- so the reconstruction is written as zeros and the SSE is sum resi^2.
    const bool allZero = chain_sync_none<LPT>( live && absSum != 0 ) && ( flags & TU_ZERO_SKIP );
    int16_t   *rec = ( recBase && live ) ? recBase + j.outOff : nullptr;
    if( allZero )
    {
      for( int i = t; i < w * h; i += LPT )
      {
        if( rec ) rec[i] = 0;
        sse_add( sse, ( int ) resi[( long ) ( i >> lw ) * j.resiStride + ( i & ( w - 1 ) )] );
      }
    }
    else
    {
      // inverse (TrQuant::xIT): tmp[i][y] = clip( sum_k blk[k][i] * M_ver[k][y] );  rec[y][x] = clip( sum_k tmp[k][y] * M_hor[k][x] )
      tuq_pass16<LPT, true>( dq16, h, reinterpret_cast<const unsigned *>( mH0 ), h - skipH, w, h, w - skipW, h, t16, 1, w, 7, t );
      chain_sync<LPT>();
      tuq_pass16<LPT, true>( t16, w, reinterpret_cast<const unsigned *>( mW ), w - skipW, h, w, h, w, rec32, w, 1, 20 - bd, t );
      chain_sync<LPT>();
      for( int i = t; i < w * h; i += LPT )
      {
        int v = rec32[i];
        if( CRS && adj ) v = lmcs_inv( v, adj, maxAbs );
        if( rec ) rec[i] = ( int16_t ) v;
        sse_add( sse, ( int ) resi[( long ) ( i >> lw ) * j.resiStride + ( i & ( w - 1 ) )] - v );   // the residual again, from L2: its LDS copy made room for a third workgroup per CU
      }
    }
  }
  long long sums[3] = { sumAbs, absSum, sse };
  chain_reduce_store<LPT, 3>( sums, sRed, sub, t, live, TuResultStore{ results + ( live ? jobIdx : 0 ) } );
}

template<int LPT, bool CRS>
int launch_tu_uni( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_tu_job *d_jobs, int n, int w, int h, int32_t *d_levelsBase, int16_t *d_recBase,
                   vtmhip_tu_result *d_results, const TrTables &tabs, int32_t *d_fwdCoefBase = nullptr )
{
  constexpr int TUS   = 256 / LPT;
  const size_t  perTu = ( size_t ) w * h + ( size_t ) w * ( h + 1 );
  const size_t  lds   = TUS * perTu * sizeof( int ) + ( ( size_t ) ( w > 32 ? 2 : 6 ) * w * w + ( w == h ? 0 : ( size_t ) ( h > 32 ? 2 : 6 ) * h * h ) ) * sizeof( int16_t );
  if( lds > 64 * 1024 )
    VTMHIP_HIP( ctx, hipFuncSetAttribute( reinterpret_cast<const void *>( tu_chain_uni_kernel<LPT, CRS> ), hipFuncAttributeMaxDynamicSharedMemorySize, ( int ) lds ) );
  VTMHIP_TIME_KERNEL( ctx, "tu_chain_uni_kernel" );
  hipLaunchKernelGGL( ( tu_chain_uni_kernel<LPT, CRS> ), dim3( ( n + TUS - 1 ) / TUS ), dim3( 256 ), lds, ctx->stream, d_resiBase, d_jobs, n, tabs, d_levelsBase, d_recBase,
                      d_results, w, h, d_fwdCoefBase, tu_chain_flags() );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

// LPT by block size: one lane = 2 x 8 outputs of a transform pass
template<bool CRS>
int launch_tu_uni_sized( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_tu_job *d_jobs, int n, int w, int h, int32_t *d_levelsBase, int16_t *d_recBase,
                         vtmhip_tu_result *d_results, const TrTables &tb, int32_t *d_fwdCoefBase )
{
  const int items = w * h / 16;
  if( items <= 4 ) return launch_tu_uni<4, CRS>( ctx, d_resiBase, d_jobs, n, w, h, d_levelsBase, d_recBase, d_results, tb, d_fwdCoefBase );
  if( items <= 8 ) return launch_tu_uni<8, CRS>( ctx, d_resiBase, d_jobs, n, w, h, d_levelsBase, d_recBase, d_results, tb, d_fwdCoefBase );
  if( items <= 16 ) return launch_tu_uni<16, CRS>( ctx, d_resiBase, d_jobs, n, w, h, d_levelsBase, d_recBase, d_results, tb, d_fwdCoefBase );
  if( items <= 32 ) return launch_tu_uni<32, CRS>( ctx, d_resiBase, d_jobs, n, w, h, d_levelsBase, d_recBase, d_results, tb, d_fwdCoefBase );
  if( items <= 64 ) return launch_tu_uni<64, CRS>( ctx, d_resiBase, d_jobs, n, w, h, d_levelsBase, d_recBase, d_results, tb, d_fwdCoefBase );
  if( items <= 128 ) return launch_tu_uni<128, CRS>( ctx, d_resiBase, d_jobs, n, w, h, d_levelsBase, d_recBase, d_results, tb, d_fwdCoefBase );
  return launch_tu_uni<256, CRS>( ctx, d_resiBase, d_jobs, n, w, h, d_levelsBase, d_recBase, d_results, tb, d_fwdCoefBase );
}

// Transform-skip candidates of a uniform batch (every job typeHor == VTMHIP_TRSKIP): elementwise, LPT = 8 lanes per TU (8 TUs per wave)
__global__ __launch_bounds__( 256 ) void tu_ts_kernel( const int16_t *__restrict__ resiBase, const vtmhip_tu_job *__restrict__ jobs, int numJobs,
                                                      int *__restrict__ levelsBase, int16_t *__restrict__ recBase, vtmhip_tu_result *__restrict__ results, int w, int h )
{
  const int jobIdx = ( blockIdx.x * 256 + threadIdx.x ) >> 3, t = threadIdx.x & 7;
  const bool live  = jobIdx < numJobs;
  const vtmhip_tu_job j = jobs[live ? jobIdx : numJobs - 1];
  const int       lw = ilog2( w );
  const QuantRule qr = quant_rule_of( j, lw, ilog2( h ), true );
  int            *levels = ( levelsBase && live ) ? levelsBase + j.outOff : nullptr;
  int16_t        *rec    = ( recBase && live ) ? recBase + j.outOff : nullptr;
  const int16_t  *resi   = resiBase + j.resiOff;
  long long sumAbs = 0, absSum = 0, sse = 0;
  for( int i = t; i < w * h; i += 8 )
  {
    const int c = resi[( long ) ( i >> lw ) * j.resiStride + ( i & ( w - 1 ) )];
    sumAbs += abs( c );
    const int q = qr.level( c, absSum );
    if( levels ) levels[i] = q;
    const int v = ( int ) ( int16_t ) qr.dequant( q );
    if( rec ) rec[i] = ( int16_t ) v;
    sse_add( sse, c - v );
  }
  long long sums[3] = { sumAbs, absSum, sse };
  chain_reduce_store<8, 3>( sums, nullptr, 0, t, live, TuResultStore{ results + ( live ? jobIdx : 0 ) } );
}

bool pow2( int v ) { return v > 0 && ( v & ( v - 1 ) ) == 0; }
int  hlog2( int v ) { int r = 0; while( ( 1 << r ) < v ) r++; return r; }

struct TuClassOf   // {8, 16, 32, 64} x {8, 16, 32, 64} with a real transform: class 4 * log2(w / 8) + log2(h / 8); everything else (4-sample sides, transform skip): the last class
{
  __device__ int operator()( const vtmhip_tu_job &j ) const
  {
    const int w = j.width, h = j.height;
    if( w < 8 || h < 8 || w > 64 || h > 64 || ( w & ( w - 1 ) ) || ( h & ( h - 1 ) ) || j.typeHor == VTMHIP_TRSKIP ) return BUCKET_OTHER;
    return 4 * ( __ffs( w ) - 4 ) + ( __ffs( h ) - 4 );
  }
};

template<bool CRS>
int tu_chain_generic( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_tu_job *d_jobs, int n, int maxWidth, int maxHeight, int32_t *d_levelsBase,
                      int16_t *d_recBase, vtmhip_tu_result *d_results )
{
  const int    mx    = maxWidth > maxHeight ? maxWidth : maxHeight;
  const size_t perTu = ( size_t ) maxWidth * maxHeight + ( size_t ) maxWidth * ( maxHeight + 1 ) + ( ( mx * mx + 1 ) >> 1 ) + ( ( maxWidth * maxHeight + 1 ) >> 1 );
  if( maxWidth * maxHeight <= 256 )
  {
    hipLaunchKernelGGL( ( tu_chain_kernel<64, CRS> ), dim3( ( n + 3 ) / 4 ), dim3( 256 ), 4 * perTu * sizeof( int ), ctx->stream, d_resiBase, d_jobs, n,
                        tabs_of( ctx ), d_levelsBase, d_recBase, d_results, maxWidth, maxHeight, tu_chain_flags() );
  }
  else
  {
    hipLaunchKernelGGL( ( tu_chain_kernel<256, CRS> ), dim3( n ), dim3( 256 ), perTu * sizeof( int ), ctx->stream, d_resiBase, d_jobs, n,
                        tabs_of( ctx ), d_levelsBase, d_recBase, d_results, maxWidth, maxHeight, tu_chain_flags() );
  }
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

// vtmhip_tu_chain_batch_dev (CRS == false) and vtmhip_tu_chain_crs_batch_dev: one dispatch, the same launch paths
template<bool CRS>
int tu_chain_entry( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_tu_job *d_jobs, int n, int maxWidth, int maxHeight, int uniformSize,
                    int32_t *d_levelsBase, int16_t *d_recBase, vtmhip_tu_result *d_results )
{
  VTMHIP_BATCH_ENTRY( ctx, n, d_resiBase && d_jobs && d_results );
  VTMHIP_REQUIRE( ctx, maxWidth >= 2 && maxWidth <= TB && maxHeight >= 2 && maxHeight <= TB, "maxWidth / maxHeight: 2..64 (2-D transforms)" );
  int st = vtmhip_internal_tr_tables( ctx );
  if( st ) return st;
  // a mixed batch with enough TUs: bucket by shape on the device (bucket.hpp), the register-blocked kernel per {8,16,32,64} x {8,16,32,64} class, the
  // generic kernel for the rest (4-sample sides, transform skip).  VTMHIP_TU_BUCKET=0 keeps the generic kernel for the whole batch.
  static const bool bucket = env_switch( "VTMHIP_TU_BUCKET", true );
  if( bucket && !uniformSize && n >= 256 && maxWidth >= 8 && maxHeight >= 8 && bucket_allowed( ctx ) )
  {
    BucketPlan plan;
    st = bucket_begin<vtmhip_tu_job, vtmhip_tu_result>( ctx, d_jobs, n, TuClassOf(), plan );
    if( st ) return st;
    for( int c = 0; c < BUCKET_CLASSES; c++ )
    {
      if( !plan.count[c] ) continue;
      const vtmhip_tu_job *jobs = ( const vtmhip_tu_job * ) plan.d_jobs + plan.offset[c];
      vtmhip_tu_result    *res  = ( vtmhip_tu_result * ) plan.d_results + plan.offset[c];
      if( c < 16 ) st = launch_tu_uni_sized<CRS>( ctx, d_resiBase, jobs, plan.count[c], 8 << ( c >> 2 ), 8 << ( c & 3 ), d_levelsBase, d_recBase, res, tabs_of( ctx ), nullptr );
      else         st = tu_chain_generic<CRS>( ctx, d_resiBase, jobs, plan.count[c], maxWidth, maxHeight, d_levelsBase, d_recBase, res );
      if( st ) return st;
    }
    return bucket_finish<vtmhip_tu_result>( ctx, plan, n, d_results );
  }
  if( uniformSize && maxWidth * maxHeight <= 32 && maxWidth >= 4 && maxHeight >= 4 )
  {
    // caller's promise: every TU is exactly maxWidth x maxHeight (4x4, 8x4 or 4x8) with a real transform -> one lane per TU
    if( maxWidth == 4 && maxHeight == 4 ) return launch_tu_lane<4, 4, CRS>( ctx, d_resiBase, d_jobs, n, d_levelsBase, d_recBase, d_results, tabs_of( ctx ) );
    if( maxWidth == 8 ) return launch_tu_lane<8, 4, CRS>( ctx, d_resiBase, d_jobs, n, d_levelsBase, d_recBase, d_results, tabs_of( ctx ) );
    return launch_tu_lane<4, 8, CRS>( ctx, d_resiBase, d_jobs, n, d_levelsBase, d_recBase, d_results, tabs_of( ctx ) );
  }
  if( uniformSize && maxWidth >= 8 && maxHeight >= 8 )
  {
    VTMHIP_REQUIRE( ctx, ( maxWidth & ( maxWidth - 1 ) ) == 0 && ( maxHeight & ( maxHeight - 1 ) ) == 0, "uniformSize: width / height must be powers of two (TU sizes are)" );
    // caller's promise: every TU is exactly maxWidth x maxHeight -> register-blocked kernel, LPT lanes per TU
    return launch_tu_uni_sized<CRS>( ctx, d_resiBase, d_jobs, n, maxWidth, maxHeight, d_levelsBase, d_recBase, d_results, tabs_of( ctx ), nullptr );
  }
  return tu_chain_generic<CRS>( ctx, d_resiBase, d_jobs, n, maxWidth, maxHeight, d_levelsBase, d_recBase, d_results );
}

struct MtsSelectArgs { double scaleSAD, fac; int numTU, numCand, maxCand; bool skip[8]; };

// TrQuant::transformNxN( tu, compID, cQP, &trModes, maxCand ) (TrQuant.cpp:950-1019) per TU: results[c * numTU + t].sumAbs -> test[c * numTU + t]
__global__ __launch_bounds__( 256 ) void mts_select_kernel( const vtmhip_tu_result *__restrict__ results, MtsSelectArgs a, uint8_t *__restrict__ test )
{
  const int t = blockIdx.x * 256 + threadIdx.x;
  if( t >= a.numTU ) return;
  int cost0 = 0, numTests = 0;
  double thr = 0.0;
  for( int c = 0; c < a.numCand; c++ )
  {
    int cost = results[( long ) c * a.numTU + t].sumAbs;
    if( a.skip[c] ) cost = ( int ) ( cost * a.scaleSAD );      // scaleSAD of the transform-skip candidate (:992-1001)
    if( c == 0 ) { cost0 = cost; thr = a.fac * cost0; }
    const bool keep = ( double ) cost <= ( c == 1 ? ( double ) cost0 : thr ) && numTests <= a.maxCand;
    test[( long ) c * a.numTU + t] = keep;
    numTests += keep;
  }
}

}   // namespace

// the dispatch of vtmhip_tu_chain_batch_dev for the other translation units of the library (sbt.hip runs its expanded sub-TU jobs through it)
int vtmhip_internal_tu_chain_launch( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_tu_job *d_jobs, int n, int maxWidth, int maxHeight, int uniformSize,
                                     int32_t *d_levelsBase, int16_t *d_recBase, vtmhip_tu_result *d_results )
{
  return tu_chain_entry<false>( ctx, d_resiBase, d_jobs, n, maxWidth, maxHeight, uniformSize, d_levelsBase, d_recBase, d_results );
}

// the same for vtmhip_tu_chain_crs_batch_dev (intra_chroma_chain.hip: jobs that carry a chroma adj)
int vtmhip_internal_tu_chain_crs_launch( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_tu_job *d_jobs, int n, int maxWidth, int maxHeight, int uniformSize,
                                         int32_t *d_levelsBase, int16_t *d_recBase, vtmhip_tu_result *d_results )
{
  return tu_chain_entry<true>( ctx, d_resiBase, d_jobs, n, maxWidth, maxHeight, uniformSize, d_levelsBase, d_recBase, d_results );
}

extern "C"
{

int vtmhip_tr_matrix_host( int type, int n, int16_t *out ) { return vtmhip_tr_matrix( type, n, out ) ? VTMHIP_E_INVALID : VTMHIP_OK; }

int vtmhip_fastFwdTrans( vtmhip_ctx *ctx, int type, int n, const int32_t *src, int32_t *dst, int shift, int line, int skipLine, int skipLine2 )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, src && dst, "null pointer" );
  VTMHIP_REQUIRE( ctx, type >= 0 && type < 3 && pow2( n ) && n >= 2 && n <= 64 && ( type == VTMHIP_DCT2 || ( n >= 4 && n <= 32 ) ),
                  "no such transform (fastFwdTrans slot is nullptr)" );
  VTMHIP_REQUIRE( ctx, line >= 1 && line <= 64 && shift >= 0 && shift < 32 && skipLine >= 0 && skipLine <= line && skipLine2 >= 0 && skipLine2 <= n, "shape" );
  VTMHIP_TRY( vtmhip_internal_tr_tables( ctx ) );
  HostStage    s( ctx );
  const size_t bytes = ( size_t ) n * line * 4, sOff = s.region( bytes ), dOff = s.region( bytes );
  VTMHIP_TRY( s.reserve() );
  memcpy( s.hp + sOff, src, bytes );
  VTMHIP_TRY( s.upload( sOff, bytes ) );
  hipLaunchKernelGGL( fwd1d_kernel, dim3( ( n * line + 255 ) / 256 ), dim3( 256 ), 0, ctx->stream, s.dev<const int>( sOff ), s.dev<int>( dOff ),
                      ctx->trTab[type][hlog2( n )], n, shift, line, skipLine, skipLine2 );
  VTMHIP_LAUNCHED( ctx );
  VTMHIP_TRY( s.fetch( dOff, bytes ) );
  memcpy( dst, s.hp + dOff, bytes );
  return VTMHIP_OK;
}

int vtmhip_fastInvTrans( vtmhip_ctx *ctx, int type, int n, const int32_t *src, int32_t *dst, int shift, int line, int skipLine, int skipLine2,
                         int32_t outputMinimum, int32_t outputMaximum )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, src && dst, "null pointer" );
  VTMHIP_REQUIRE( ctx, type >= 0 && type < 3 && pow2( n ) && n >= 2 && n <= 64 && ( type == VTMHIP_DCT2 || ( n >= 4 && n <= 32 ) ),
                  "no such transform (fastInvTrans slot is nullptr)" );
  VTMHIP_REQUIRE( ctx, line >= 1 && line <= 64 && shift >= 1 && shift < 32 && skipLine >= 0 && skipLine <= line && skipLine2 >= 0 && skipLine2 <= n, "shape" );
  VTMHIP_TRY( vtmhip_internal_tr_tables( ctx ) );
  HostStage    s( ctx );
  const size_t bytes = ( size_t ) n * line * 4, sOff = s.region( bytes ), dOff = s.region( bytes );
  VTMHIP_TRY( s.reserve() );
  memcpy( s.hp + sOff, src, bytes );
  VTMHIP_TRY( s.upload( sOff, bytes ) );
  hipLaunchKernelGGL( inv1d_kernel, dim3( ( n * line + 255 ) / 256 ), dim3( 256 ), 0, ctx->stream, s.dev<const int>( sOff ), s.dev<int>( dOff ),
                      ctx->trTab[type][hlog2( n )], n, shift, line, skipLine, skipLine2, outputMinimum, outputMaximum );
  VTMHIP_LAUNCHED( ctx );
  VTMHIP_TRY( s.fetch( dOff, bytes ) );
  memcpy( dst, s.hp + dOff, bytes );
  return VTMHIP_OK;
}

int vtmhip_xT_batch_dev( vtmhip_ctx *ctx, const int16_t *d_resiBase, int32_t *d_coefBase, const vtmhip_tr_job *d_jobs, int n, int maxWidth,
                         int maxHeight, int32_t *d_sumAbs )
{
  VTMHIP_BATCH_ENTRY( ctx, n, d_resiBase && d_coefBase && d_jobs );
  VTMHIP_REQUIRE( ctx, maxWidth >= 1 && maxWidth <= TB && maxHeight >= 1 && maxHeight <= TB, "maxWidth / maxHeight (max transform size 64)" );
  int st = vtmhip_internal_tr_tables( ctx );
  if( st ) return st;
  const int    mx  = maxWidth > maxHeight ? maxWidth : maxHeight;
  const size_t lds = ( size_t ) ( maxWidth * maxHeight + maxWidth * ( maxHeight + 1 ) ) * 4 + ( size_t ) mx * mx * 2 + 16;
  hipLaunchKernelGGL( xT_kernel, dim3( n ), dim3( 256 ), lds, ctx->stream, d_resiBase, d_coefBase, d_jobs, tabs_of( ctx ), d_sumAbs );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

int vtmhip_xIT_batch_dev( vtmhip_ctx *ctx, const int32_t *d_coefBase, int16_t *d_resiBase, const vtmhip_tr_job *d_jobs, int n, int maxWidth,
                          int maxHeight )
{
  VTMHIP_BATCH_ENTRY( ctx, n, d_resiBase && d_coefBase && d_jobs );
  VTMHIP_REQUIRE( ctx, maxWidth >= 1 && maxWidth <= TB && maxHeight >= 1 && maxHeight <= TB, "maxWidth / maxHeight (max transform size 64)" );
  int st = vtmhip_internal_tr_tables( ctx );
  if( st ) return st;
  const int    mx  = maxWidth > maxHeight ? maxWidth : maxHeight;
  const size_t lds = ( size_t ) ( 2 * maxWidth * maxHeight ) * 4 + ( size_t ) mx * mx * 2 + 16;
  hipLaunchKernelGGL( xIT_kernel, dim3( n ), dim3( 256 ), lds, ctx->stream, d_coefBase, d_resiBase, d_jobs, tabs_of( ctx ) );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

int vtmhip_quant_batch_dev( vtmhip_ctx *ctx, const int32_t *d_coefBase, int32_t *d_qBase, int32_t *d_deltaUBase, const vtmhip_quant_job *d_jobs, int n,
                            int32_t *d_absSum )
{
  VTMHIP_BATCH_ENTRY( ctx, n, d_coefBase && d_qBase && d_jobs && d_absSum );
  hipLaunchKernelGGL( quant_kernel, dim3( n ), dim3( 256 ), 0, ctx->stream, d_coefBase, d_qBase, d_deltaUBase, d_jobs, d_absSum );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

int vtmhip_dequant_batch_dev( vtmhip_ctx *ctx, const int32_t *d_qBase, int32_t *d_coefBase, const vtmhip_quant_job *d_jobs, int n )
{
  VTMHIP_BATCH_ENTRY( ctx, n, d_coefBase && d_qBase && d_jobs );
  hipLaunchKernelGGL( dequant_kernel, dim3( n ), dim3( 256 ), 0, ctx->stream, d_qBase, d_coefBase, d_jobs );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

int vtmhip_tu_chain_batch_dev( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_tu_job *d_jobs, int n, int maxWidth, int maxHeight,
                               int uniformSize, int32_t *d_levelsBase, int16_t *d_recBase, vtmhip_tu_result *d_results )
{
  return tu_chain_entry<false>( ctx, d_resiBase, d_jobs, n, maxWidth, maxHeight, uniformSize, d_levelsBase, d_recBase, d_results );
}

int vtmhip_tu_chain_crs_batch_dev( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_tu_job *d_jobs, int n, int maxWidth, int maxHeight,
                                   int uniformSize, int32_t *d_levelsBase, int16_t *d_recBase, vtmhip_tu_result *d_results )
{
  return tu_chain_entry<true>( ctx, d_resiBase, d_jobs, n, maxWidth, maxHeight, uniformSize, d_levelsBase, d_recBase, d_results );
}

int vtmhip_tu_ts_chain_batch_dev( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_tu_job *d_jobs, int n, int width, int height,
                                  int32_t *d_levelsBase, int16_t *d_recBase, vtmhip_tu_result *d_results )
{
  VTMHIP_BATCH_ENTRY( ctx, n, d_resiBase && d_jobs && d_results );
  VTMHIP_REQUIRE( ctx, pow2( width ) && pow2( height ) && width >= 4 && height >= 4 && width <= 32 && height <= 32, "transform skip: 4..32 (log2MaxTransformSkipBlockSize)" );
  VTMHIP_TIME_KERNEL( ctx, "tu_ts_kernel" );
  hipLaunchKernelGGL( tu_ts_kernel, dim3( ( n + 31 ) / 32 ), dim3( 256 ), 0, ctx->stream, d_resiBase, d_jobs, n, d_levelsBase, d_recBase, d_results, width, height );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

// The same selection from RAW sums: mtsIdx[i] is the candidate's tu.mtsIdx (MTS_DCT2_DCT2 = 0, MTS_SKIP = 1, MTS_DST7_DST7 = 2 ...); the sum of a
// transform-skip candidate (sum |residual|) is scaled here as the reference scales it (:992-1001): int( sumAbs * scaleSAD ) with scaleSAD =
// 2^trShift, times 1/1.414213562 when log2(width) + log2(height) is odd.
int vtmhip_mts_select2( const int32_t *sumAbs, const uint8_t *mtsIdx, int numCand, int width, int height, int bitDepth, int maxLog2TrDynamicRange, int maxCand,
                        uint8_t *test )
{
  if( !sumAbs || !mtsIdx || !test || numCand < 1 || numCand > 16 || width < 1 || height < 1 ) return VTMHIP_E_INVALID;
  int lw = 0, lh = 0;
  while( ( 2 << lw ) <= width ) lw++;
  while( ( 2 << lh ) <= height ) lh++;
  int32_t scaled[16];
  for( int i = 0; i < numCand; i++ )
  {
    scaled[i] = sumAbs[i];
    if( mtsIdx[i] == 1 )
    {
      double scaleSAD = 1.0;
      if( ( lw + lh ) & 1 ) scaleSAD = 1.0 / 1.414213562;
      const int trShift = maxLog2TrDynamicRange - bitDepth - ( ( lw + lh ) >> 1 );
      scaleSAD *= pow( 2, trShift );
      scaled[i] = ( int ) ( sumAbs[i] * scaleSAD );
    }
  }
  return vtmhip_mts_select( scaled, numCand, width, height, maxCand, test );
}

// the same rule for every TU of a level, one thread per TU (fp64 compare as the reference: facBB[] x the first candidate's cost)
int vtmhip_mts_select_batch_dev( vtmhip_ctx *ctx, const vtmhip_tu_result *d_results, int numTU, int numCand, const uint8_t *mtsIdx, int width, int height,
                                 int bitDepth, int maxLog2TrDynamicRange, int maxCand, uint8_t *d_test )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, numTU >= 0 && numCand >= 1 && numCand <= 8 && width >= 4 && height >= 4 && mtsIdx, "numTU / numCand / size" );
  if( numTU == 0 ) return VTMHIP_OK;
  VTMHIP_REQUIRE( ctx, d_results && d_test, "null pointer" );
  int lw = 0, lh = 0;
  while( ( 2 << lw ) <= width ) lw++;
  while( ( 2 << lh ) <= height ) lh++;
  MtsSelectArgs a;
  for( int i = 0; i < 8; i++ ) a.skip[i] = i < numCand && mtsIdx[i] == 1;
  a.scaleSAD = ( ( lw + lh ) & 1 ) ? 1.0 / 1.414213562 : 1.0;
  a.scaleSAD *= pow( 2, maxLog2TrDynamicRange - bitDepth - ( ( lw + lh ) >> 1 ) );
  static const double facBB[] = { 1.2, 1.3, 1.3, 1.4, 1.5 };
  const int lg = lw > lh ? lw : lh;
  a.fac = facBB[lg - 2 > 0 ? ( lg - 2 > 4 ? 4 : lg - 2 ) : 0];
  a.numTU = numTU; a.numCand = numCand; a.maxCand = maxCand;
  hipLaunchKernelGGL( mts_select_kernel, dim3( ( numTU + 255 ) / 256 ), dim3( 256 ), 0, ctx->stream, d_results, a, d_test );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

// MTS candidate pre-selection thresholds (TrQuant::transformNxN( ..., trModes, maxCand ), TrQuant.cpp:950-1019): host arithmetic (fp64).
// sumAbs[i]: sum |coef| of candidate i in trModes order, as vtmhip_xT_batch_dev returns it (a transform-skip candidate already scaled by
// the caller, :992-1001).  The reference compares the candidate at LIST POSITION 1 against the unscaled threshold (:1012).
// test[i] = 1 when the candidate survives.
int vtmhip_mts_select( const int32_t *sumAbs, int numCand, int width, int height, int maxCand, uint8_t *test )
{
  if( !sumAbs || !test || numCand < 1 || width < 1 || height < 1 ) return VTMHIP_E_INVALID;
  static const double facBB[] = { 1.2, 1.3, 1.3, 1.4, 1.5 };
  const int    mx  = width > height ? width : height;
  int          lg  = 0;
  while( ( 2 << lg ) <= mx ) lg++;
  const int    fi  = lg - 2 > 0 ? ( lg - 2 > 4 ? 4 : lg - 2 ) : 0;
  const double thr = facBB[fi] * sumAbs[0], thrTS = sumAbs[0];
  int          numTests = 0;
  for( int i = 0; i < numCand; i++ )
  {
    const bool t = sumAbs[i] <= ( i == 1 ? thrTS : thr ) && numTests <= maxCand;
    test[i]      = t;
    numTests += t;
  }
  return VTMHIP_OK;
}

}   // extern "C"


extern "C" int vtmhip_xT_uniform_batch_dev( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_tu_job *d_jobs, int n, int width, int height, int32_t *d_coefBase,
                                            vtmhip_tu_result *d_results )
{
  VTMHIP_BATCH_ENTRY( ctx, n, d_resiBase && d_jobs && d_coefBase && d_results );
  VTMHIP_REQUIRE( ctx, width >= 8 && width <= TB && height >= 8 && height <= TB && pow2( width ) && pow2( height ), "width / height: powers of two 8..64" );
  int st = vtmhip_internal_tr_tables( ctx );
  if( st ) return st;
  return launch_tu_uni_sized<false>( ctx, d_resiBase, d_jobs, n, width, height, nullptr, nullptr, d_results, tabs_of( ctx ), d_coefBase );
}


// =====================================================================================================================
// LFNST kernels (TrQuant::fwdLfnstNxN / invLfnstNxN, TrQuant.cpp:233-311): a 16 x 16 or 16 x 48 int8 matrix-vector product per TU.
// One wave per job.  Forward: lane = part * 16 + j, four lanes share output j (12 or 4 of the 48 / 16 products each).
// Inverse: lane j < trSize sums its column over the first zeroOutSize rows.  The matrices come from the caller (vtmhip_lfnst_set_tables).
// =====================================================================================================================
namespace
{
__global__ __launch_bounds__( 256 ) void lfnst_kernel( const int8_t *__restrict__ tab, const int *__restrict__ srcBase, int *__restrict__ dstBase,
                                                      const vtmhip_lfnst_job *__restrict__ jobs, int n )
{
  const int lane = threadIdx.x & 63;
  const int job  = blockIdx.x * 4 + ( threadIdx.x >> 6 );
  if( job >= n ) return;
  const vtmhip_lfnst_job j = jobs[job];
  const int     trSize = j.size > 4 ? 48 : 16, zo = j.zeroOutSize;
  const int8_t *M   = j.size > 4 ? tab + ( ( j.mode * 2 + j.index ) * 16 ) * 48 : tab + 4 * 2 * 16 * 48 + ( ( j.mode * 2 + j.index ) * 16 ) * 16;
  const int    *src = srcBase + j.srcOff;
  int          *dst = dstBase + j.dstOff;
  if( !j.inverse )
  {
    const int o = lane & 15, part = lane >> 4, per = trSize >> 2;
    int       acc = 0;
    if( o < zo )
      for( int i = part * per; i < ( part + 1 ) * per; i++ ) acc += src[i] * ( int ) M[o * trSize + i];
    acc += __shfl_xor( acc, 16, 64 );
    acc += __shfl_xor( acc, 32, 64 );
    if( lane < trSize ) dst[lane] = lane < zo ? ( acc + 64 ) >> 7 : 0;   // lanes 16..47 of the 8x8 case write the zeroed tail
    return;
  }
  if( lane < trSize )
  {
    int acc = 0;
    for( int i = 0; i < zo; i++ ) acc += src[i] * ( int ) M[i * trSize + lane];
    dst[lane] = min( 32767, max( -32768, ( acc + 64 ) >> 7 ) );
  }
}

// TrQuant::xFwdLfnst / xInvLfnst (TrQuant.cpp:340-420, 422-527) on a TU's coefficient block IN PLACE: the low-frequency region is gathered
// (row-major, or transposed for the intra modes past the diagonal), multiplied with the 16 x 16 / 16 x 48 core matrix and written back along the
// coefficient scan (forward) -- or the reverse.  The scan positions are the first 16 / 48 of the diagonal scan in 4x4 coefficient groups
// (g_scanOrder[SCAN_GROUPED_4x4][SCAN_DIAG] / g_coefTopLeftDiagScan8x8): generated here, checked against the reference's tables in the tests.
__device__ __forceinline__ int lfnst_scan_pos( int k, int width, bool sb8 )   // k-th scan position -> index x + y * width
{
  // inside a 4x4 group: up-right diagonals, each from bottom-left to top-right; groups of the 8x8 region in the same diagonal order: (0,0), (0,1), (1,0), (1,1)
  const int g = k >> 4, i = k & 15;
  const int dx[16] = { 0, 0, 1, 0, 1, 2, 0, 1, 2, 3, 1, 2, 3, 2, 3, 3 }, dy[16] = { 0, 1, 0, 2, 1, 0, 3, 2, 1, 0, 3, 2, 1, 3, 2, 3 };
  const int gx = sb8 ? ( g == 2 || g == 3 ) : 0, gy = sb8 ? ( g == 1 || g == 3 ) : 0;
  return ( gx * 4 + dx[i] ) + ( gy * 4 + dy[i] ) * width;
}

__global__ __launch_bounds__( 256 ) void lfnst_tu_kernel( const int8_t *__restrict__ tab, int *__restrict__ coefBase, const vtmhip_lfnst_tu_job *__restrict__ jobs, int n )
{
  __shared__ int sIn[4][48], sOut[4][48];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int job  = blockIdx.x * 4 + wv;
  if( job >= n ) return;
  const vtmhip_lfnst_tu_job j = jobs[job];
  const int  w = j.width, h = j.height;
  const bool sb8 = w >= 8 && h >= 8;
  const int  sbSize = sb8 ? 8 : 4, trSize = sb8 ? 48 : 16, zo = ( ( w == 4 && h == 4 ) || ( w == 8 && h == 8 ) ) ? 8 : 16;
  const int8_t *M = sb8 ? tab + ( ( j.mode * 2 + j.index ) * 16 ) * 48 : tab + 4 * 2 * 16 * 48 + ( ( j.mode * 2 + j.index ) * 16 ) * 16;
  int *coef = coefBase + j.coefOff;
  // region position r (0 .. trSize-1) of the LFNST input / output vector -> (x, y) in the block
  auto region_xy = [&]( int r, int &x, int &y ) {
    int row, col;
    if( sbSize == 4 ) { row = r >> 2; col = r & 3; }
    else if( r < 32 ) { row = r >> 3; col = r & 7; }
    else { row = 4 + ( ( r - 32 ) >> 2 ); col = ( r - 32 ) & 3; }
    // transposed gather: lfnstTemp[col' * sbSize(or 4) ...]: the vector index of block position (x, y) is that of (y, x) in the untransposed layout
    if( j.transpose ) { x = row; y = col; } else { x = col; y = row; }
  };
  if( !j.inverse )
  {
    if( lane < trSize ) { int x, y; region_xy( lane, x, y ); sIn[wv][lane] = coef[y * w + x]; }
    __builtin_amdgcn_fence( __ATOMIC_ACQ_REL, "wavefront" ); __builtin_amdgcn_wave_barrier();
    if( lane < trSize )
    {
      int acc = 0;
      if( lane < zo ) { for( int i = 0; i < trSize; i++ ) acc += sIn[wv][i] * ( int ) M[lane * trSize + i]; acc = ( acc + 64 ) >> 7; }
      sOut[wv][lane] = lane < zo ? acc : 0;
    }
    __builtin_amdgcn_fence( __ATOMIC_ACQ_REL, "wavefront" ); __builtin_amdgcn_wave_barrier();
    if( lane < trSize ) coef[lfnst_scan_pos( lane, w, sb8 )] = sOut[wv][lane];
  }
  else
  {
    if( lane < 16 ) sIn[wv][lane] = coef[lfnst_scan_pos( lane, w, sb8 )];
    __builtin_amdgcn_fence( __ATOMIC_ACQ_REL, "wavefront" ); __builtin_amdgcn_wave_barrier();
    if( lane < trSize )
    {
      int acc = 0;
      for( int i = 0; i < zo; i++ ) acc += sIn[wv][i] * ( int ) M[i * trSize + lane];
      int x, y; region_xy( lane, x, y );
      coef[y * w + x] = min( 32767, max( -32768, ( acc + 64 ) >> 7 ) );
    }
  }
}
}   // namespace

extern "C"
{

int vtmhip_lfnst_tu_batch_dev( vtmhip_ctx *ctx, int32_t *d_coefBase, const vtmhip_lfnst_tu_job *d_jobs, int n )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, n >= 0, "n" );
  if( n == 0 ) return VTMHIP_OK;
  VTMHIP_REQUIRE( ctx, ctx->lfnstTab, "vtmhip_lfnst_set_tables has not been called" );
  VTMHIP_REQUIRE( ctx, d_coefBase && d_jobs, "null pointer" );
  hipLaunchKernelGGL( lfnst_tu_kernel, dim3( ( n + 3 ) / 4 ), dim3( 256 ), 0, ctx->stream, ctx->lfnstTab, d_coefBase, d_jobs, n );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

int vtmhip_lfnst_scan_host( int width, int height, int32_t *pos48 )
{
  if( !pos48 || width < 4 || height < 4 ) return VTMHIP_E_INVALID;
  const bool sb8 = width >= 8 && height >= 8;
  static const int dx[16] = { 0, 0, 1, 0, 1, 2, 0, 1, 2, 3, 1, 2, 3, 2, 3, 3 }, dy[16] = { 0, 1, 0, 2, 1, 0, 3, 2, 1, 0, 3, 2, 1, 3, 2, 3 };
  for( int k = 0; k < ( sb8 ? 48 : 16 ); k++ )
  {
    const int g = k >> 4, i = k & 15, gx = sb8 ? ( g == 2 || g == 3 ) : 0, gy = sb8 ? ( g == 1 || g == 3 ) : 0;
    pos48[k] = ( gx * 4 + dx[i] ) + ( gy * 4 + dy[i] ) * width;
  }
  return VTMHIP_OK;
}

int vtmhip_lfnst_set_tables( vtmhip_ctx *ctx, const int8_t *lfnst8x8, const int8_t *lfnst4x4 )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, lfnst8x8 && lfnst4x4, "null pointer" );
  const size_t n8 = 4 * 2 * 16 * 48, n4 = 4 * 2 * 16 * 16;
  if( !ctx->lfnstTab ) VTMHIP_HIP( ctx, hipMalloc( ( void ** ) &ctx->lfnstTab, n8 + n4 ) );
  VTMHIP_HIP( ctx, hipMemcpyAsync( ctx->lfnstTab, lfnst8x8, n8, hipMemcpyHostToDevice, ctx->stream ) );
  VTMHIP_HIP( ctx, hipMemcpyAsync( ctx->lfnstTab + n8, lfnst4x4, n4, hipMemcpyHostToDevice, ctx->stream ) );
  VTMHIP_HIP( ctx, hipStreamSynchronize( ctx->stream ) );   // the host arrays may go away
  return VTMHIP_OK;
}

int vtmhip_lfnst_batch_dev( vtmhip_ctx *ctx, const int32_t *d_srcBase, int32_t *d_dstBase, const vtmhip_lfnst_job *d_jobs, int n )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, n >= 0, "n" );
  if( n == 0 ) return VTMHIP_OK;
  VTMHIP_REQUIRE( ctx, ctx->lfnstTab, "vtmhip_lfnst_set_tables has not been called" );
  VTMHIP_REQUIRE( ctx, d_srcBase && d_dstBase && d_jobs, "null pointer" );
  hipLaunchKernelGGL( lfnst_kernel, dim3( ( n + 3 ) / 4 ), dim3( 256 ), 0, ctx->stream, ctx->lfnstTab, d_srcBase, d_dstBase, d_jobs, n );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

static int lfnst_single( vtmhip_ctx *ctx, const int32_t *src, int32_t *dst, int mode, int index, int size, int zeroOutSize, int inverse )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, src && dst, "null pointer" );
  VTMHIP_REQUIRE( ctx, ctx->lfnstTab, "vtmhip_lfnst_set_tables has not been called" );
  VTMHIP_REQUIRE( ctx, mode >= 0 && mode < 4 && index >= 0 && index < 2 && ( size == 4 || size == 8 ) && ( zeroOutSize == 8 || zeroOutSize == 16 ), "mode / index / size / zeroOutSize" );
  const int trSize = size > 4 ? 48 : 16, nIn = inverse ? zeroOutSize : trSize;
  HostStage    s( ctx );
  const size_t srcOff = s.region( sizeof( int32_t ) * 48 ), dstOff = s.region( sizeof( int32_t ) * 48 ), jobOff = s.region( sizeof( vtmhip_lfnst_job ) );
  VTMHIP_TRY( s.reserve() );
  memcpy( s.hp + srcOff, src, sizeof( int32_t ) * nIn );
  vtmhip_lfnst_job j;
  memset( &j, 0, sizeof( j ) );
  j.srcOff = ( int64_t ) ( srcOff / 4 ); j.dstOff = ( int64_t ) ( dstOff / 4 ); j.mode = ( uint8_t ) mode; j.index = ( uint8_t ) index; j.size = ( uint8_t ) size; j.zeroOutSize = ( uint8_t ) zeroOutSize; j.inverse = ( uint8_t ) inverse;
  s.put( jobOff, j );
  VTMHIP_TRY( s.upload( 0, s.total ) );
  hipLaunchKernelGGL( lfnst_kernel, dim3( 1 ), dim3( 256 ), 0, ctx->stream, ctx->lfnstTab, s.dev<const int>( 0 ), s.dev<int>( 0 ), s.dev<const vtmhip_lfnst_job>( jobOff ), 1 );
  VTMHIP_LAUNCHED( ctx );
  VTMHIP_TRY( s.fetch( dstOff, sizeof( int32_t ) * trSize ) );
  memcpy( dst, s.hp + dstOff, sizeof( int32_t ) * trSize );
  return VTMHIP_OK;
}

int vtmhip_fwdLfnstNxN( vtmhip_ctx *ctx, const int32_t *src, int32_t *dst, int mode, int index, int size, int zeroOutSize )
{
  return lfnst_single( ctx, src, dst, mode, index, size, zeroOutSize, 0 );
}
int vtmhip_invLfnstNxN( vtmhip_ctx *ctx, const int32_t *src, int32_t *dst, int mode, int index, int size, int zeroOutSize )
{
  return lfnst_single( ctx, src, dst, mode, index, size, zeroOutSize, 1 );
}

}   // extern "C"
