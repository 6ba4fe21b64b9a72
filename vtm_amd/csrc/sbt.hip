// sbt.hip -- sub-block transform (SBT) of inter CUs on the device; the rules are sbt_rules.hpp's.
//   vtmhip_sbt_est_batch_dev    InterSearch::calcMinDistSbt for a batch of CUs               (EncoderLib/InterSearch.cpp:6195-6387)
//   vtmhip_sbt_skip_by_rdcost   InterSearch::skipSbtByRDCost, host arithmetic                (:6389-6438)
//   vtmhip_sbt_chain_batch_dev  the SBT candidates of xEstimateInterResidualQT: expansion into sub-TU jobs, the fused chain of transform.hip through its own
//                               dispatch, and the completion of the candidate over the whole CU
//
// sbt_est_kernel<L>: a CU gets L lanes (16: four CUs share a wave; 64: a wave; 256: the workgroup), chosen by the host from the batch's largest CU.  A lane walks
// the component block in row-major pairs of samples (one 4-byte load per plane; a pair never straddles a partition: a partition is at least 2 samples wide),
// keeps the running sum of the partition it is in and adds it to the CU's 3 x 16 table in LDS when the partition changes -- a handful of LDS atomics per lane,
// no cross-lane reduction.  Lane 0 of the CU then runs sbtCombine and writes the record.
//
// sbt_finish_kernel: a wave per (candidate, component).  The chain has left the compact sub-TU reconstruction at the head of the CU-shaped block; the wave
// stages it in LDS, then writes the whole block (coded tile from LDS, zero elsewhere) and sums the uncoded tile's residual on the way.
//
// The chain entry reads its job table back through HostStage and lays its workspace out with a WorkPlan in the slot VTMHIP_WORK_SBT (stage.hpp).
#include "ctx.hpp"
#include "stage.hpp"
#include "sbt_rules.hpp"
#include "pel_pack.hpp"

namespace
{

__host__ __device__ inline bool sbt_side_ok( int s ) { return s >= 4 && s <= 64 && ( s & ( s - 1 ) ) == 0; }
__host__ __device__ inline int  sbt_log2( int v ) { int r = 0; while( ( 1 << r ) < v ) r++; return r; }

__host__ __device__ inline bool sbt_est_job_ok( const vtmhip_sbt_est_job &j )
{
  if( !sbt_side_ok( j.width ) || !sbt_side_ok( j.height ) || j.bitDepth < 8 || j.bitDepth > 12 ) return false;
  return ( j.sbtAllowed & ~sbtAllowed( j.width, j.height, 64 ) ) == 0;
}

template<int L>
__global__ __launch_bounds__( 256 ) void sbt_est_kernel( const int16_t *__restrict__ orgBase, const int16_t *__restrict__ predBase,
                                                         const vtmhip_sbt_est_job *__restrict__ jobs, int n, vtmhip_sbt_est_result *__restrict__ results )
{
  constexpr int G = 256 / L;
  __shared__ unsigned sPart[G][48];   // [component][j][i]
  for( int i = threadIdx.x; i < G * 48; i += 256 ) ( &sPart[0][0] )[i] = 0;
  __syncthreads();

  const int g = threadIdx.x / L, l = threadIdx.x % L, job = blockIdx.x * G + g;
  bool      valid = job < n;
  vtmhip_sbt_est_job j;
  if( valid )
  {
    j     = jobs[job];
    valid = sbt_est_job_ok( j );
  }
  const int npx = valid ? sbtNumPart( j.width ) : 1, npy = valid ? sbtNumPart( j.height ) : 1;
  if( valid )
  {
    const int shift = sbtDistShift( j.bitDepth );
    for( int c = 0; c < 3; c++ )
    {
      if( c && ( j.orgOff[1] < 0 || j.orgOff[2] < 0 || j.predOff[1] < 0 || j.predOff[2] < 0 ) ) break;
      const int cw = c ? j.width >> 1 : j.width, ch = c ? j.height >> 1 : j.height;
      const int lgHalf = sbt_log2( cw ) - 1, lgLenX = sbt_log2( cw / npx ), lgLenY = sbt_log2( ch / npy ), pairs = ( cw >> 1 ) * ch;
      const int16_t *o = orgBase + j.orgOff[c], *p = predBase + j.predOff[c];
      const int      os = j.orgStride[c], ps = j.predStride[c];
      int      cur = -1;
      unsigned acc = 0;
      for( int idx = l; idx < pairs; idx += L )
      {
        const int y = idx >> lgHalf, x = ( idx & ( ( 1 << lgHalf ) - 1 ) ) << 1;
        const int part = ( ( y >> lgLenY ) << 2 ) + ( x >> lgLenX );
        const unsigned a = reinterpret_cast<const Pel2 *>( o + ( long ) y * os + x )->v, b = reinterpret_cast<const Pel2 *>( p + ( long ) y * ps + x )->v;
        const int d0 = ( short ) ( a & 0xffffu ) - ( short ) ( b & 0xffffu ), d1 = ( ( int ) a >> 16 ) - ( ( int ) b >> 16 );
        if( part != cur )
        {
          if( cur >= 0 ) atomicAdd( &sPart[g][c * 16 + cur], acc );
          cur = part;
          acc = 0;
        }
        acc += ( ( ( unsigned ) d0 * ( unsigned ) d0 ) >> shift ) + ( ( ( unsigned ) d1 * ( unsigned ) d1 ) >> shift );   // unsigned: the square of any int16 difference fits 32 bits
      }
      if( cur >= 0 ) atomicAdd( &sPart[g][c * 16 + cur], acc );
    }
  }
  __syncthreads();
  if( !valid || l ) return;

  vtmhip_sbt_est_result &r = results[job];
  uint64_t dist[4][4];
#pragma unroll
  for( int jj = 0; jj < 4; jj++ )
#pragma unroll
    for( int ii = 0; ii < 4; ii++ )
    {
      const bool in = jj < npy && ii < npx;
      uint64_t   d  = 0;
#pragma unroll
      for( int c = 0; c < 3; c++ )
      {
        const unsigned u = in ? sPart[g][c * 16 + jj * 4 + ii] : 0;
        r.part[c][jj][ii] = u;
        d += c ? ( uint64_t ) ( double( ( uint64_t ) u ) * j.chromaWeight ) : ( uint64_t ) u;
      }
      dist[jj][ii] = d;
    }
  uint64_t est[9];
  uint8_t  order[8];
  r.skipAll = ( uint8_t ) sbtCombine( dist, npx, npy, j.sbtAllowed, j.distScale, est, order );
#pragma unroll
  for( int m = 0; m < 9; m++ ) r.est[m] = est[m];
#pragma unroll
  for( int m = 0; m < 8; m++ ) r.rdoOrder[m] = order[m];
#pragma unroll
  for( int m = 0; m < 7; m++ ) r.pad[m] = 0;
}

// ---- the candidate chain ------------------------------------------------------------------------------------------------------------------------
__host__ __device__ inline bool sbt_job_ok( const vtmhip_sbt_job &j )
{
  if( !sbt_side_ok( j.width ) || !sbt_side_ok( j.height ) || j.bitDepth < 8 || j.bitDepth > 12 || j.sbtPos > 1 ) return false;
  if( !targetSbtAllowed( j.sbtIdx, sbtAllowed( j.width, j.height, 64 ) ) || j.resiOff[0] < 0 ) return false;
  for( int c = 0; c < 3; c++ )
    if( ( c == 0 || j.resiOff[c] >= 0 ) && ( j.qpRem[c] < 0 || j.qpRem[c] > 5 || j.qpPer[c] < 0 ) ) return false;
  return true;
}

__host__ __device__ inline bool sbt_has( const vtmhip_sbt_job &j, int c ) { return c == 0 || j.resiOff[c] >= 0; }

// the sub-TU of component c as a job of the fused chain
__host__ __device__ inline void sbt_expand( const vtmhip_sbt_job &j, int c, vtmhip_tu_job &t )
{
  const int cw = c ? j.width >> 1 : j.width, ch = c ? j.height >> 1 : j.height;
  int       x, y, w, h, trHor = SBT_TR_DCT2, trVer = SBT_TR_DCT2;
  sbtCodedTile( cw, ch, j.sbtIdx, j.sbtPos, x, y, w, h );
  if( c == 0 ) sbtTrTypes( j.sbtIdx, j.sbtPos, w, h, trHor, trVer );
  t.resiOff    = j.resiOff[c] + ( int64_t ) y * j.resiStride[c] + x;
  t.outOff     = j.outOff[c];
  t.resiStride = j.resiStride[c];
  t.width = ( int16_t ) w; t.height = ( int16_t ) h;
  t.qpPer = j.qpPer[c]; t.qpRem = j.qpRem[c];
  t.typeHor = ( uint8_t ) trHor; t.typeVer = ( uint8_t ) trVer;   // SBT_TR_* are VTMHIP_DCT2 / DCT8 / DST7
  t.bitDepth = j.bitDepth; t.isIRAP = j.isIRAP;
  t.pad = 0; t.chromaAdj = 0;
}
static_assert( SBT_TR_DCT2 == VTMHIP_DCT2 && SBT_TR_DCT8 == VTMHIP_DCT8 && SBT_TR_DST7 == VTMHIP_DST7, "transform type codes" );

// job i -> tuJobs[i] (luma) and, for its chroma components, the next free slots from n on (a wave reserves its slots with one atomic; the order among waves is
// whatever the atomics give: every sub-TU is independent and tuIdx leads each result back to its candidate)
__global__ __launch_bounds__( 256 ) void sbt_expand_kernel( const vtmhip_sbt_job *__restrict__ jobs, int n, int *__restrict__ cursor, vtmhip_tu_job *__restrict__ tuJobs,
                                                            int *__restrict__ tuIdx )
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
  vtmhip_sbt_job j;
  bool cb = false, cr = false;
  if( i < n )
  {
    j  = jobs[i];
    cb = sbt_has( j, 1 );
    cr = sbt_has( j, 2 );
  }
  const unsigned long long mCb = __ballot( cb ), mCr = __ballot( cr ), below = ( 1ull << lane ) - 1;
  int base = 0;
  if( lane == 0 ) base = atomicAdd( cursor, __popcll( mCb ) + __popcll( mCr ) );
  base = __shfl( base, 0, 64 );
  if( i >= n ) return;
  const int slotCb = n + base + __popcll( mCb & below ) + __popcll( mCr & below ), slotCr = slotCb + ( cb ? 1 : 0 );
  sbt_expand( j, 0, tuJobs[i] );
  tuIdx[3 * i] = i;
  if( cb ) sbt_expand( j, 1, tuJobs[slotCb] );
  if( cr ) sbt_expand( j, 2, tuJobs[slotCr] );
  tuIdx[3 * i + 1] = cb ? slotCb : -1;
  tuIdx[3 * i + 2] = cr ? slotCr : -1;
}

template<typename T> __device__ __forceinline__ T sbt_pick( const T ( &a )[3], int c ) { return c == 0 ? a[0] : c == 1 ? a[1] : a[2]; }   // keeps the job in registers

constexpr int SBT_MAX_TU = 2048;   // the largest sub-TU: 32 x 64 samples (half of a 64 x 64 CU)

__global__ __launch_bounds__( 256 ) void sbt_finish_kernel( const int16_t *__restrict__ resiBase, const vtmhip_sbt_job *__restrict__ jobs, int n, const int *__restrict__ tuIdx,
                                                            const vtmhip_tu_result *__restrict__ tuRes, int16_t *recBase, vtmhip_sbt_result *__restrict__ results )
{
  __shared__ int16_t sRec[4][SBT_MAX_TU];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63, item = blockIdx.x * 4 + wv, cand = item / 3, c = item - 3 * cand;
  const int idx = cand < n ? tuIdx[item] : -1;
  int       cw = 0, ch = 0, tx = 0, ty = 0, tw = 0, th = 0;
  vtmhip_sbt_job j;
  int16_t *rec = nullptr;
  if( idx >= 0 )
  {
    j  = jobs[cand];
    cw = c ? j.width >> 1 : j.width;
    ch = c ? j.height >> 1 : j.height;
    sbtCodedTile( cw, ch, j.sbtIdx, j.sbtPos, tx, ty, tw, th );
    if( recBase )
    {
      rec = recBase + sbt_pick( j.outOff, c );
      for( int i = lane; i < tw * th; i += 64 ) sRec[wv][i] = rec[i];
    }
  }
  __syncthreads();   // every lane's reads of the compact block are done before any lane overwrites the block
  if( cand >= n ) return;
  unsigned long long zero = 0;
  if( idx >= 0 )
  {
    const int16_t *resi = resiBase + sbt_pick( j.resiOff, c );
    const int      lgW = sbt_log2( cw ), lgTw = sbt_log2( tw ), shift = sbtDistShift( j.bitDepth ), stride = sbt_pick( j.resiStride, c );
    unsigned       acc = 0;
    for( int i = lane; i < cw * ch; i += 64 )
    {
      const int  y = i >> lgW, x = i & ( cw - 1 );
      const bool coded = x >= tx && x < tx + tw && y >= ty && y < ty + th;
      if( !coded )
      {
        const int r = resi[( long ) y * stride + x];
        acc += ( unsigned ) ( r * r ) >> shift;
      }
      if( rec ) rec[i] = coded ? sRec[wv][( ( y - ty ) << lgTw ) + ( x - tx )] : ( int16_t ) 0;
    }
    zero = wave_reduce_add_u64( acc );
  }
  if( lane == 0 )
  {
    vtmhip_sbt_result &r = results[cand];
    r.sseCoded[c] = idx >= 0 ? tuRes[idx].sse : 0;
    r.sseZero[c]  = zero;
    r.absSum[c]   = idx >= 0 ? tuRes[idx].absSum : 0;
    if( c == 0 ) r.pad = 0;
  }
}

// the host pass both entries share: checks every job, counts the sub-TUs and their largest sides
int sbt_scan_jobs( const vtmhip_sbt_job *jobs, int n, int &numTu, int &maxW, int &maxH )
{
  numTu = 0; maxW = maxH = 2;
  for( int i = 0; i < n; i++ )
  {
    const vtmhip_sbt_job &j = jobs[i];
    if( !sbt_job_ok( j ) ) return VTMHIP_E_INVALID;
    for( int c = 0; c < 3; c++ )
    {
      if( !sbt_has( j, c ) ) continue;
      int x, y, w, h;
      sbtCodedTile( c ? j.width >> 1 : j.width, c ? j.height >> 1 : j.height, j.sbtIdx, j.sbtPos, x, y, w, h );
      if( w > maxW ) maxW = w;
      if( h > maxH ) maxH = h;
      numTu++;
    }
  }
  return VTMHIP_OK;
}

}   // namespace

extern "C"
{

int vtmhip_sbt_struct_size( int which )
{
  switch( which )
  {
  case 0: return ( int ) sizeof( vtmhip_sbt_est_job );
  case 1: return ( int ) sizeof( vtmhip_sbt_est_result );
  case 2: return ( int ) sizeof( vtmhip_sbt_job );
  case 3: return ( int ) sizeof( vtmhip_sbt_result );
  default: return -1;
  }
}

int vtmhip_sbt_est_batch_dev( vtmhip_ctx *ctx, const int16_t *d_orgBase, const int16_t *d_predBase, const vtmhip_sbt_est_job *d_jobs, int n, int maxWidth,
                              int maxHeight, vtmhip_sbt_est_result *d_results )
{
  VTMHIP_BATCH_ENTRY( ctx, n, d_orgBase && d_predBase && d_jobs && d_results );
  VTMHIP_REQUIRE( ctx, maxWidth >= 4 && maxWidth <= 64 && maxHeight >= 4 && maxHeight <= 64, "maxWidth / maxHeight: 4 .. 64" );
  VTMHIP_TIME_KERNEL( ctx, "sbt_est_kernel" );
  const int area = maxWidth * maxHeight;
  if( area <= 256 ) hipLaunchKernelGGL( sbt_est_kernel<16>, dim3( ( n + 15 ) / 16 ), dim3( 256 ), 0, ctx->stream, d_orgBase, d_predBase, d_jobs, n, d_results );
  else if( area <= 1024 ) hipLaunchKernelGGL( sbt_est_kernel<64>, dim3( ( n + 3 ) / 4 ), dim3( 256 ), 0, ctx->stream, d_orgBase, d_predBase, d_jobs, n, d_results );
  else hipLaunchKernelGGL( sbt_est_kernel<256>, dim3( n ), dim3( 256 ), 0, ctx->stream, d_orgBase, d_predBase, d_jobs, n, d_results );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

int vtmhip_sbt_skip_by_rdcost( const uint64_t est[9], double distScale, int sbtIdx, int sbtPos, double bestCost, uint64_t distSbtOff, double costSbtOff,
                               int rootCbfSbtOff )
{
  if( !est || sbtIdx < SBT_VER_HALF || sbtIdx > SBT_HOR_QUAD || sbtPos < 0 || sbtPos > 1 ) return VTMHIP_E_INVALID;
  return sbtSkipByRdCost( est, distScale, sbtIdx, sbtPos, bestCost, distSbtOff, costSbtOff, rootCbfSbtOff );
}

int vtmhip_sbt_make_tu_jobs( const vtmhip_sbt_job *jobs, int n, vtmhip_tu_job *out, int *numOut, int32_t *tuIdx )
{
  if( n < 0 || !numOut || ( n && ( !jobs || !out ) ) ) return VTMHIP_E_INVALID;
  int numTu, maxW, maxH;
  if( sbt_scan_jobs( jobs, n, numTu, maxW, maxH ) ) return VTMHIP_E_INVALID;
  int next = n;
  for( int i = 0; i < n; i++ )
    for( int c = 0; c < 3; c++ )
    {
      const int slot = !sbt_has( jobs[i], c ) ? -1 : c ? next++ : i;
      if( slot >= 0 ) sbt_expand( jobs[i], c, out[slot] );
      if( tuIdx ) tuIdx[3 * i + c] = slot;
    }
  *numOut = numTu;
  return VTMHIP_OK;
}

int vtmhip_sbt_chain_batch_dev( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_sbt_job *d_jobs, int n, int32_t *d_levelsBase, int16_t *d_recBase,
                                vtmhip_sbt_result *d_results )
{
  VTMHIP_BATCH_ENTRY( ctx, n, d_resiBase && d_jobs && d_results );
  // the job table decides the launches (sub-TU count, largest sides) and is checked before anything runs
  HostStage             hs( ctx );
  const vtmhip_sbt_job *jobs = nullptr;
  VTMHIP_TRY( hs.pull_table( d_jobs, n, jobs ) );
  int numTu, maxW, maxH;
  VTMHIP_REQUIRE( ctx, sbt_scan_jobs( jobs, n, numTu, maxW, maxH ) == VTMHIP_OK,
                  "sbt job: sides 4..64 (powers of two), a mode the size allows, sbtPos 0..1, bitDepth 8..12, qpRem 0..5, qpPer >= 0, luma offset >= 0" );

  // workspace: the slot cursor, tuIdx[3 n], the expanded jobs, their results
  WorkPlan     wp;
  const size_t oCursor = wp.region<int>( 1 ), oIdx = wp.region<int>( ( size_t ) 3 * n ), oJobs = wp.region<vtmhip_tu_job>( numTu ), oRes = wp.region<vtmhip_tu_result>( numTu );
  VTMHIP_TRY( wp.reserve( ctx, VTMHIP_WORK_SBT ) );
  int              *d_cursor = wp.at<int>( oCursor ), *d_tuIdx = wp.at<int>( oIdx );
  vtmhip_tu_job    *d_tuJobs = wp.at<vtmhip_tu_job>( oJobs );
  vtmhip_tu_result *d_tuRes  = wp.at<vtmhip_tu_result>( oRes );
  VTMHIP_HIP( ctx, hipMemsetAsync( d_cursor, 0, sizeof( int ), ctx->stream ) );
  hipLaunchKernelGGL( sbt_expand_kernel, dim3( ( n + 255 ) / 256 ), dim3( 256 ), 0, ctx->stream, d_jobs, n, d_cursor, d_tuJobs, d_tuIdx );
  VTMHIP_LAUNCHED( ctx );
  VTMHIP_TRY( vtmhip_internal_tu_chain_launch( ctx, d_resiBase, d_tuJobs, numTu, maxW, maxH, 0, d_levelsBase, d_recBase, d_tuRes ) );
  VTMHIP_TIME_KERNEL( ctx, "sbt_finish_kernel" );
  hipLaunchKernelGGL( sbt_finish_kernel, dim3( ( 3 * n + 3 ) / 4 ), dim3( 256 ), 0, ctx->stream, d_resiBase, d_jobs, n, d_tuIdx, d_tuRes, d_recBase, d_results );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

}   // extern "C"
