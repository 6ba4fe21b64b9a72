// lfnst_chain.hip -- the lfnstIdx 1 / 2 candidates of an intra luma TU in one kernel; the rules are lfnst_rules.hpp's, the quant rule, the group synchronisation and the
// reduction tu_stages.hpp's.
//   vtmhip_lfnst_chain_batch_dev   xT restricted to the kept region -> xFwdLfnst -> Quant::quant over 8 / 16 scan positions -> Quant::dequant -> xInvLfnst -> xIT with the
//                                  same zero-out -> SSE( residual, reconstructed residual )     (CommonLib/TrQuant.cpp:339-526, 776-923, Quant.cpp:955-1038)
//   vtmhip_lfnst_mode_host         set index and transpose flag of a prediction
//   vtmhip_internal_lfnst_expand_launch / vtmhip_internal_lfnst_chain_launch   what vtmhip_intra_chain_lfnst_batch_dev (intra_chain.hip) launches
//
// lfnst_chain_kernel<LANES>: a job gets LANES lanes (16: sixteen jobs per workgroup, the largest job of the table has up to 256 samples; 64: a wave per job), so a
// group lies inside one wave and every step meets at chain_sync -- no workgroup barrier.  Per job in LDS (lfnstJobInts): the int16 residual, which the SSE reads
// again; the keep x ( H + 1 ) block between the two passes of a transform; keep rows of the W- and of the H-point DCT-2 matrix, transposed for the forward passes and
// restaged plain for the inverse ones; the keep x keep region; the 16 / 48 vector of the core multiply; 16 dequantised values; the levels of the top-left 4x4.
// The passes are lean forms of tu_stages.hpp's lds_fwd_pass / lds_inv_pass -- same sums, same rounding, same clip -- that neither stage nor walk the matrix rows and
// lines the zero-out drops: keep = 4 or 8 of N frequencies per dimension.  A group past the end of the table repeats the last job in its own slot and stores nothing.
// The entry reads its job table back through HostStage (stage.hpp) and checks it before anything runs.
#include "ctx.hpp"
#include "stage.hpp"
#include "tu_stages.hpp"
#include "lfnst_rules.hpp"

namespace
{

struct Dct2Tabs { const int16_t *m[7]; };   // [log2 N] -> the N x N forward DCT-2 matrix (row-major), the context's

__device__ __forceinline__ void lfnst_sse_add( long long &sse, int d ) { sse += ( long long ) ( unsigned long long ) ( ( unsigned ) d * ( unsigned ) d ); }

template<int LANES>
__global__ __launch_bounds__( 256 ) void lfnst_chain_kernel( const int8_t *__restrict__ tab, const int16_t *__restrict__ resiBase, const vtmhip_lfnst_chain_job *__restrict__ jobs,
                                                            int numJobs, Dct2Tabs tabs, int jobInts, int *__restrict__ levelsBase, int16_t *__restrict__ recBase,
                                                            vtmhip_tu_result *__restrict__ results )
{
  extern __shared__ __attribute__( ( aligned( 16 ) ) ) int ldsw[];
  constexpr int G = 256 / LANES;
  const int  sub = threadIdx.x / LANES, t = threadIdx.x % LANES, jobIdx = blockIdx.x * G + sub;
  const bool live = jobIdx < numJobs;
  const vtmhip_lfnst_chain_job j = jobs[live ? jobIdx : numJobs - 1];
  const int  w = j.width, h = j.height, bd = j.bitDepth, lw = ilog2( w ), lh = ilog2( h );
  const bool sb8 = w >= 8 && h >= 8, transpose = j.transpose != 0;
  const int  keep = sb8 ? 8 : 4, lk = sb8 ? 3 : 2, zo = lfnstZeroOut( w, h ), trSize = sb8 ? 48 : 16, ld = h + 1, ldr = w + 2;
  int       *slot = ldsw + sub * jobInts;
  int16_t   *sR   = ( int16_t * ) slot;                  // [h][w + 2] the residual
  int       *tmp  = slot + ( ( ldr * h ) >> 1 );         // [keep][h + 1]
  int16_t   *sMw  = ( int16_t * ) ( tmp + keep * ld );   // keep rows of the W-point matrix, then of the H-point one
  int16_t   *sMh  = sMw + keep * w;
  int       *reg  = tmp + keep * ld + ( ( keep * ( w + h ) ) >> 1 );   // [keep][keep] the region
  int       *vec  = reg + 64, *dqv = vec + 48, *lvl = dqv + 16;
  const int16_t *resi = resiBase + j.resiOff, *mw = tabs.m[lw], *mh = tabs.m[lh];
  const int8_t  *M = sb8 ? tab + ( ( j.setIdx * 2 + j.index ) * 16 ) * 48 : tab + 4 * 2 * 16 * 48 + ( ( j.setIdx * 2 + j.index ) * 16 ) * 16;

  for( int i = t; i < w * h; i += LANES ) sR[( i >> lw ) * ldr + ( i & ( w - 1 ) )] = resi[( long ) ( i >> lw ) * j.resiStride + ( i & ( w - 1 ) )];
  for( int i = t; i < keep * w; i += LANES ) sMw[( i & ( w - 1 ) ) * keep + ( i >> lw )] = mw[i];   // sMw[n * keep + k] = M[k][n]
  for( int i = t; i < keep * h; i += LANES ) sMh[( i & ( h - 1 ) ) * keep + ( i >> lh )] = mh[i];
  if( t < 16 ) lvl[t] = 0;
  chain_sync<LANES>();

  // forward, TrQuant::xT: tmp[k][y] for the keep horizontal frequencies, then reg[k2][k] for the keep vertical ones
  {
    const int s1 = lw + bd + 6 - 15, s2 = lh + 6;
    for( int o = t; o < keep * h; o += LANES )
    {
      const int y = o >> lk, k = o & ( keep - 1 );
      unsigned  sum = 0;
      for( int n = 0; n < w; n++ ) sum += ( unsigned ) ( int ) sR[y * ldr + n] * ( unsigned ) ( int ) sMw[n * keep + k];
      tmp[k * ld + y] = ( int ) ( sum + ( 1u << ( s1 - 1 ) ) ) >> s1;
    }
    chain_sync<LANES>();
    for( int o = t; o < keep * keep; o += LANES )
    {
      const int k = o >> lk, k2 = o & ( keep - 1 );
      unsigned  sum = 0;
      for( int y = 0; y < h; y++ ) sum += ( unsigned ) tmp[k * ld + y] * ( unsigned ) ( int ) sMh[y * keep + k2];
      reg[k2 * keep + k] = ( int ) ( sum + ( 1u << ( s2 - 1 ) ) ) >> s2;
    }
    chain_sync<LANES>();
  }

  // TrQuant::xFwdLfnst: gather (transposed when flagged), fwdLfnstNxN; four lanes share an output when the group is a wave
  for( int v = t; v < trSize; v += LANES )
  {
    int x, y;
    lfnstRegionXY( v, sb8, transpose, x, y );
    vec[v] = reg[y * keep + x];
  }
  chain_sync<LANES>();
  constexpr int PARTS = LANES / 16;
  int           acc = 0;
  {
    const int oj = t & 15, part = t >> 4, per = trSize / PARTS;
    if( oj < zo )
      for( int i = part * per; i < ( part + 1 ) * per; i++ ) acc += vec[i] * ( int ) M[oj * trSize + i];
    if( PARTS == 4 )
    {
      acc += __shfl_xor( acc, 16, 64 );
      acc += __shfl_xor( acc, 32, 64 );
    }
  }
  // Quant::quant on the first zo scan positions, which lie in the top-left 4x4, and Quant::dequant
  long long sumAbs = 0, absSum = 0, sse = 0;
  if( t < zo )
  {
    const QuantRule qr = quant_rule( bd, j.qpPer, j.qpRem, j.isIRAP, lw, lh, false );
    const int       c = ( acc + 64 ) >> 7;
    sumAbs += abs( c );
    const int q = qr.level( c, absSum );
    lvl[lfnstScanPos( t, 4, false )] = q;
    dqv[t] = qr.dequant( q );
  }
  // the forward matrices are done with: the same rows plain for the inverse passes
  for( int i = t; i < keep * w; i += LANES ) sMw[i] = mw[i];
  for( int i = t; i < keep * h; i += LANES ) sMh[i] = mh[i];
  chain_sync<LANES>();

  if( levelsBase && live )
  {
    int *levels = levelsBase + j.outOff;
    for( int i = t; i < w * h; i += LANES )
    {
      const int y = i >> lw, x = i & ( w - 1 );
      levels[i] = ( x < 4 && y < 4 ) ? lvl[y * 4 + x] : 0;
    }
  }
  // TrQuant::xInvLfnst: invLfnstNxN with its clip, scattered back to the region; the bottom-right 4x4 of an 8x8 region is zero
  for( int v = t; v < keep * keep; v += LANES )
  {
    int x, y, val = 0;
    if( v < trSize )
    {
      int a = 0;
      for( int i = 0; i < zo; i++ ) a += dqv[i] * ( int ) M[i * trSize + v];
      val = clip16( ( a + 64 ) >> 7 );
      lfnstRegionXY( v, sb8, transpose, x, y );
    }
    else { x = 4 + ( ( v - 48 ) & 3 ); y = 4 + ( ( v - 48 ) >> 2 ); }
    reg[y * keep + x] = val;
  }
  chain_sync<LANES>();

  // inverse, TrQuant::xIT with cut = keep: tmp[i][y] for the keep columns, then every sample, and the SSE against the residual
  for( int o = t; o < keep * h; o += LANES )
  {
    const int i = o >> lh, y = o & ( h - 1 );
    unsigned  sum = 0;
    for( int k = 0; k < keep; k++ ) sum += ( unsigned ) reg[k * keep + i] * ( unsigned ) ( int ) sMh[k * h + y];
    tmp[i * ld + y] = clip16( ( int ) ( sum + 64u ) >> 7 );
  }
  chain_sync<LANES>();
  {
    const int s = 20 - bd;
    int16_t  *rec = ( recBase && live ) ? recBase + j.outOff : nullptr;
    for( int o = t; o < w * h; o += LANES )
    {
      const int y = o >> lw, x = o & ( w - 1 );
      unsigned  sum = 0;
      for( int k = 0; k < keep; k++ ) sum += ( unsigned ) tmp[k * ld + y] * ( unsigned ) ( int ) sMw[k * w + x];
      const int v = clip16( ( int ) ( sum + ( 1u << ( s - 1 ) ) ) >> s );
      if( rec ) rec[o] = ( int16_t ) v;
      lfnst_sse_add( sse, ( int ) sR[y * ldr + x] - ( int ) ( int16_t ) v );
    }
  }
  long long sums[3] = { sumAbs, absSum, sse };
  vtmhip_tu_result *res = results + ( live ? jobIdx : 0 );
  chain_reduce_store<LANES, 3>( sums, ( long long ( * )[3] ) nullptr, sub, t, live, [res]( const long long ( &v )[3] ) {
    vtmhip_tu_result r;
    r.sse = ( uint64_t ) v[2]; r.sumAbs = ( int32_t ) v[0]; r.absSum = ( int32_t ) v[1];
    *res = r;
  } );
}

// one thread per LFNST job of the level entry: the chain's job, its mirror as a vtmhip_tu_job (what intra_chain_finish_kernel reads: offsets, shape, bit depth) and
// the block index
__global__ __launch_bounds__( 256 ) void lfnst_expand_kernel( const vtmhip_intra_block *__restrict__ blocks, const vtmhip_intra_job *__restrict__ intraJobs, int nIntra,
                                                             const vtmhip_mip_job *__restrict__ mipJobs, const vtmhip_intra_lfnst_tu_job *__restrict__ lfnstJobs, int n,
                                                             vtmhip_lfnst_chain_job *__restrict__ out, vtmhip_tu_job *__restrict__ mirror, int *__restrict__ tuBlock )
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if( i >= n ) return;
  vtmhip_lfnst_chain_job c;
  int                    blk;
  lfnstExpandAt( blocks, intraJobs, nIntra, mipJobs, lfnstJobs[i], c, blk );
  out[i] = c;
  vtmhip_tu_job m;
  m.resiOff = c.resiOff; m.outOff = c.outOff; m.resiStride = c.resiStride;
  m.width = c.width; m.height = c.height; m.qpPer = c.qpPer; m.qpRem = c.qpRem;
  m.typeHor = VTMHIP_DCT2; m.typeVer = VTMHIP_DCT2; m.bitDepth = c.bitDepth; m.isIRAP = c.isIRAP;
  m.pad = 0; m.chromaAdj = 0;
  mirror[i]  = m;
  tuBlock[i] = blk;
}

}   // namespace

int vtmhip_internal_lfnst_expand_launch( vtmhip_ctx *ctx, const vtmhip_intra_block *d_blocks, const vtmhip_intra_job *d_intraJobs, int nIntra, const vtmhip_mip_job *d_mipJobs,
                                         const vtmhip_intra_lfnst_tu_job *d_lfnstJobs, int n, vtmhip_lfnst_chain_job *d_out, vtmhip_tu_job *d_mirror, int *d_tuBlock )
{
  VTMHIP_TIME_KERNEL( ctx, "lfnst_expand_kernel" );
  hipLaunchKernelGGL( lfnst_expand_kernel, dim3( ( n + 255 ) / 256 ), dim3( 256 ), 0, ctx->stream, d_blocks, d_intraJobs, nIntra, d_mipJobs, d_lfnstJobs, n, d_out, d_mirror,
                      d_tuBlock );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

// the chain's launch alone, its jobs checked by the caller: maxArea and jobInts are the LfnstPlan of the table
int vtmhip_internal_lfnst_chain_launch( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_lfnst_chain_job *d_jobs, int n, int maxArea, int jobInts,
                                        int32_t *d_levelsBase, int16_t *d_recBase, vtmhip_tu_result *d_results )
{
  VTMHIP_REQUIRE( ctx, ctx->lfnstTab, "vtmhip_lfnst_set_tables has not been called" );
  VTMHIP_TRY( vtmhip_internal_tr_tables( ctx ) );
  Dct2Tabs tabs;
  for( int l = 0; l < 7; l++ ) tabs.m[l] = ctx->trTab[VTMHIP_DCT2][l];
  const int    lanes = lfnstLanes( maxArea ), perGroup = 256 / lanes;
  const size_t lds = ( size_t ) perGroup * jobInts * sizeof( int );   // at most 16 x 2.9 KB or 4 x 13.2 KB
  VTMHIP_REQUIRE( ctx, lds <= 64 * 1024, "LFNST chain: LDS plan" );
  VTMHIP_TIME_KERNEL( ctx, "lfnst_chain_kernel" );
  if( lanes == 16 )
    hipLaunchKernelGGL( lfnst_chain_kernel<16>, dim3( ( n + perGroup - 1 ) / perGroup ), dim3( 256 ), lds, ctx->stream, ctx->lfnstTab, d_resiBase, d_jobs, n, tabs, jobInts,
                        d_levelsBase, d_recBase, d_results );
  else
    hipLaunchKernelGGL( lfnst_chain_kernel<64>, dim3( ( n + perGroup - 1 ) / perGroup ), dim3( 256 ), lds, ctx->stream, ctx->lfnstTab, d_resiBase, d_jobs, n, tabs, jobInts,
                        d_levelsBase, d_recBase, d_results );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

extern "C"
{

int vtmhip_lfnst_chain_struct_size( int which )
{
  switch( which )
  {
  case 0: return ( int ) sizeof( vtmhip_lfnst_chain_job );
  case 1: return ( int ) sizeof( vtmhip_intra_lfnst_tu_job );
  default: return -1;
  }
}

int vtmhip_lfnst_chain_lanes_per_job( int maxArea ) { return lfnstLanes( maxArea ); }

int vtmhip_lfnst_mode_host( int width, int height, int intraMode, int isMip, int *setIdx, int *transpose )
{
  if( !setIdx || !transpose || !lfnstShapeOk( width, height, isMip != 0 ) ) return VTMHIP_E_INVALID;
  if( !isMip && ( intraMode < 0 || intraMode >= INTRA_NUM_LUMA_MODE ) ) return VTMHIP_E_INVALID;
  lfnstModeOf( width, height, intraMode, isMip != 0, *setIdx, *transpose );
  return VTMHIP_OK;
}

int vtmhip_lfnst_chain_batch_dev( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_lfnst_chain_job *d_jobs, int n, int32_t *d_levelsBase, int16_t *d_recBase,
                                  vtmhip_tu_result *d_results )
{
  VTMHIP_BATCH_ENTRY( ctx, n, d_resiBase && d_jobs && d_results );
  VTMHIP_REQUIRE( ctx, ctx->lfnstTab, "vtmhip_lfnst_set_tables has not been called" );
  // the kernel trusts its jobs: the table is read back and checked before anything runs
  HostStage                     hs( ctx );
  const vtmhip_lfnst_chain_job *jobs = nullptr;
  VTMHIP_TRY( hs.pull_table( d_jobs, n, jobs ) );
  LfnstPlan plan;
  VTMHIP_REQUIRE( ctx, lfnstChainScan( jobs, n, plan ),
                  "LFNST chain jobs: sides 4..64, resiStride >= width, bitDepth 8..12, qpRem 0..5, qpPer >= 0, setIdx 0..3, index 0..1, transpose 0..1, pad 0" );
  return vtmhip_internal_lfnst_chain_launch( ctx, d_resiBase, d_jobs, n, plan.maxArea, plan.jobInts, d_levelsBase, d_recBase, d_results );
}

}   // extern "C"
