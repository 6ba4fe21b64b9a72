// jccr.hip -- joint Cb-Cr residual coding (JCCR / ICT): the forward / inverse inter-component transform and the joint chroma candidate of the residual loop.
//
// Reference: CommonLib/TrQuant.cpp fwdTransformCbCr / invTransformCbCr :86-157 (the tables m_fwdICT / m_invICT[-3..3] :166-181), fwdTransformICT /
// invTransformICT / selectICTCandidates :619-687; g_ictModes CommonLib/Rom.cpp:527; TU::getICTMode CommonLib/UnitTools.cpp:3825; the joint loop of
// xEstimateInterResidualQT, EncoderLib/InterSearch.cpp:6813-7032 (forward ICT :6851, transformNxN on the coded component :6884-6890, invTransformNxN +
// invTransformICT :6964-6975, DF_SSE of Cb and Cr against the original residuals :6984-6998).
//
// The chain kernels run the stages of the single-component chain (tu_stages.hpp: the same definitions transform.hip's tu_chain_kernel / tu_chain_lane_kernel /
// tu_chain_uni_kernel call) between a forward ICT at the load and an inverse ICT + two SSEs at the end; chroma joint candidates are DCT2 / DCT2 or transform
// skip, so only the DCT-2 matrices are staged.
//
// Headroom: a joint residual is a Pel, so every path takes the whole int16 range.  The generic and the lane kernel multiply and accumulate in 32 bits like the
// reference; the register-blocked kernel's packed passes are exact for it too (tu_stages.hpp states the bound).  The residuals an encoder produces stay far
// below: 6 (2^bitDepth - 1) / 5.
//
// CRS (template flag of the three chain kernels, vtmhip_jccr_chain_crs_batch_dev): LMCS chroma residual scaling around the joint candidate (InterSearch.cpp:6822-6823,
// 6838-6842, 6977-6998) with lmcs.hpp's rules -- Cb and Cr go through fwd() before the forward ICT (fwdDist is the distance on the scaled pair), both rebuilt blocks
// through inv() before the rec stores and the SSEs, which are taken against the unscaled residuals.  The job's adj is 0 for "leave this job alone".
//
// Out of scope: ACT, the picture-level sign decision (the caller passes signFlag), the CABAC estimate.
//
// The chain entries read their job table back through HostStage (stage.hpp), as the other chains' entries do.
#include "ctx.hpp"
#include "stage.hpp"
#include "lmcs.hpp"
#include "tu_stages.hpp"

namespace
{

struct DctTabs { const int16_t *m[7]; };   // [log2 N] -> device pointer to the N x N forward DCT-2 matrix (row-major)

// ---- the ICT rules ---------------------------------------------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ int ict_abs_mode( int cbfMask ) { return cbfMask == 1 ? 3 : cbfMask - 1; }   // |g_ictModes[.][cbfMask]|, cbfMask 1 .. 3

// the joint residual of one sample: C++ division (toward zero), then the Pel wrap
__device__ __forceinline__ int ict_fwd( int am, int s, int cb, int cr )
{
  const int v = am == 1 ? ( 4 * cb + s * 2 * cr ) / 5 : am == 2 ? ( cb + s * cr ) / 2 : ( 4 * cr + s * 2 * cb ) / 5;
  return ( int ) ( int16_t ) v;
}

// the component the decoder derives from the coded one (v: a Pel)
__device__ __forceinline__ int ict_inv( int am, int s, int v )
{
  if( am == 2 ) return s > 0 ? v : ( v == -32768 ? 32767 : -v );   // the non-normative clip of mode -2
  return ( s * v ) >> 1;
}

__device__ __forceinline__ long long ict_dist( int am, int s, int cb, int cr, int c )
{
  const int       o  = am == 2 ? s * c : ( s * c ) >> 1;   // (the forward distance of mode -2 knows no clip: square( crx + c1 ))
  const long long e0 = am == 3 ? cb - o : cb - c, e1 = am == 3 ? cr - c : cr - o;
  return e0 * e0 + e1 * e1;
}

// one reconstructed sample v of the coded component: both rebuilt blocks and both squared errors against the original residuals
// (CRS: both go through the inverse scaling first; cb, cr are the UNSCALED residuals)
template<bool CRS>
__device__ __forceinline__ void jccr_finish( int am, int s, int v, int cb, int cr, int16_t *recCb, int16_t *recCr, long i, long long &sseCb, long long &sseCr, int adj,
                                             int maxAbs )
{
  const int o = ict_inv( am, s, v );
  int       rb = am == 3 ? o : v, rr = am == 3 ? v : o;
  if( CRS && adj ) { rb = lmcs_inv( rb, adj, maxAbs ); rr = lmcs_inv( rr, adj, maxAbs ); }
  if( recCb ) recCb[i] = ( int16_t ) rb;
  if( recCr ) recCr[i] = ( int16_t ) rr;
  const int db = cb - rb, dr = cr - rr;
  sseCb += ( long long ) ( unsigned long long ) ( ( unsigned ) db * ( unsigned ) db );
  sseCr += ( long long ) ( unsigned long long ) ( ( unsigned ) dr * ( unsigned ) dr );
}

// CRS: the job's effective adj (0: not scaled), the clip bound and the reciprocal of the forward rule
struct CrsParams { int adj, maxAbs; LmcsScale sc; };

template<bool CRS>
__device__ __forceinline__ CrsParams crs_params( const vtmhip_jccr_job &j, int w, int h )
{
  CrsParams p;
  p.adj    = CRS ? lmcs_job_adj( j.chromaAdj, w, h ) : 0;
  p.maxAbs = ( 1 << j.bitDepth ) - 1;
  p.sc     = lmcs_scale_of( CRS && p.adj ? p.adj : 1 );
  return p;
}

// the (Cb, Cr) pair as the forward ICT sees it
template<bool CRS>
__device__ __forceinline__ void crs_fwd_pair( const CrsParams &p, int &cb, int &cr )
{
  if( CRS && p.adj ) { cb = lmcs_fwd( cb, p.sc, p.maxAbs ); cr = lmcs_fwd( cr, p.sc, p.maxAbs ); }
}

__device__ __forceinline__ QuantRule quant_rule_of( const vtmhip_jccr_job &j, int lw, int lh, bool ts ) { return quant_rule( j.bitDepth, j.qpPer, j.qpRem, j.isIRAP, lw, lh, ts ); }

// ---- forward ICT of all four cbfMasks: one wave per (Cb, Cr) pair --------------------------------------------------------------------------------------
__global__ __launch_bounds__( 256 ) void ict_fwd_kernel( const int16_t *__restrict__ resiBase, const vtmhip_ict_job *__restrict__ jobs, int n,
                                                        int16_t *__restrict__ jointBase, long long *__restrict__ dist )
{
  const int lane = threadIdx.x & 63, job = blockIdx.x * 4 + ( threadIdx.x >> 6 );
  if( job >= n ) return;
  const vtmhip_ict_job j = jobs[job];
  const int      w = j.width, h = j.height, s = j.signFlag ? -1 : 1;
  const int16_t *cb = resiBase + j.cbOff, *cr = resiBase + j.crOff;
  int16_t       *out = jointBase ? jointBase + j.outOff : nullptr;
  long long      d[5] = { 0, 0, 0, 0, 0 };   // sum cb^2, sum cr^2, d1 of cbfMask 1, 2, 3
  for( int i = lane; i < w * h; i += 64 )
  {
    const int y = i / w, x = i - y * w;
    const int b = cb[( long ) y * j.cbStride + x], r = cr[( long ) y * j.crStride + x];
    d[0] += ( long long ) b * b;
    d[1] += ( long long ) r * r;
#pragma unroll
    for( int m = 1; m <= 3; m++ )
    {
      const int am = ict_abs_mode( m ), c = ict_fwd( am, s, b, r );
      d[1 + m] += ict_dist( am, s, b, r, c );
      if( out && ( ( j.maskBits >> m ) & 1 ) ) out[( long ) ( m - 1 ) * w * h + i] = ( int16_t ) c;
    }
  }
#pragma unroll
  for( int k = 0; k < 5; k++ ) d[k] = ( long long ) wave_reduce_add_u64( ( unsigned long long ) d[k] );
  if( lane == 0 )
  {
    long long *o = dist + ( long ) job * 8;
    o[0] = d[0]; o[1] = d[1];
    o[2] = d[2]; o[3] = 0;
    o[4] = d[3]; o[5] = 0;
    o[6] = d[4]; o[7] = 0;
  }
}

// inverse ICT in place on two contiguous blocks (the pointer entry)
__global__ __launch_bounds__( 256 ) void ict_inv_kernel( int16_t *__restrict__ cb, int16_t *__restrict__ cr, int count, int am, int s )
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if( i >= count ) return;
  if( am == 3 ) cb[i] = ( int16_t ) ict_inv( am, s, cr[i] );
  else cr[i] = ( int16_t ) ict_inv( am, s, cb[i] );
}

// ---- the joint chain, generic path: everything in LDS, TPT threads per pair (64: four independent pairs per workgroup, wave-level synchronisation only;
// 256: one pair per workgroup) -- tu_chain_kernel between the two ICTs ---------------------------------------------------------------------------------
struct JccrSums { long long sumAbs, absSum, sseCb, sseCr, fwdDist; };

__device__ __forceinline__ vtmhip_jccr_result jccr_result_of( const JccrSums &a )
{
  vtmhip_jccr_result r;
  r.sseCb = ( uint64_t ) a.sseCb; r.sseCr = ( uint64_t ) a.sseCr; r.fwdDist = a.fwdDist; r.sumAbs = ( int32_t ) a.sumAbs; r.absSum = ( int32_t ) a.absSum;
  return r;
}

// the five sums over the TPT threads of a pair
template<int TPT>
__device__ __forceinline__ void jccr_reduce_store( const JccrSums &a, long long ( *sRed )[5], int sub, int t, bool live, vtmhip_jccr_result *out )
{
  long long v[5] = { a.sumAbs, a.absSum, a.sseCb, a.sseCr, a.fwdDist };
  chain_reduce_store<TPT, 5>( v, sRed, sub, t, live, [out]( const long long ( &r )[5] ) { const JccrSums rs = { r[0], r[1], r[2], r[3], r[4] }; *out = jccr_result_of( rs ); } );
}

template<int TPT, bool CRS>
__global__ __launch_bounds__( 256 ) void jccr_chain_kernel( const int16_t *__restrict__ resiBase, const vtmhip_jccr_job *__restrict__ jobs, int numJobs, DctTabs tabs,
                                                           int *__restrict__ levelsBase, int16_t *__restrict__ recCbBase, int16_t *__restrict__ recCrBase,
                                                           vtmhip_jccr_result *__restrict__ results, int maxW, int maxH )
{
  extern __shared__ __attribute__( ( aligned( 16 ) ) ) int ldsw[];
  __shared__ long long sRed[4][5];
  constexpr int TUS = 256 / TPT;
  const int     sub = TPT == 64 ? ( int ) ( threadIdx.x >> 6 ) : 0, t = TPT == 64 ? ( int ) ( threadIdx.x & 63 ) : ( int ) threadIdx.x;
  const int     jobIdx = blockIdx.x * TUS + sub;
  if( jobIdx >= numJobs ) return;   // TPT == 64: whole waves leave; TPT == 256: grid == numJobs
  const vtmhip_jccr_job j = jobs[jobIdx];
  const int      w = j.width, h = j.height, bd = j.bitDepth;
  const int      mx = maxW > maxH ? maxW : maxH;
  const int      perTu = maxW * maxH + maxW * ( maxH + 1 ) + ( ( mx * mx + 1 ) >> 1 );   // ints
  int           *blk = ldsw + sub * perTu;            // [h][w] joint residual -> coefficients -> dequantised coefficients
  int           *tmp = blk + maxW * maxH;             // [w][h+1] / [w][h]
  int16_t       *sM  = ( int16_t * ) ( tmp + maxW * ( maxH + 1 ) );
  const int16_t *cbp = resiBase + j.cbOff, *crp = resiBase + j.crOff;
  const int      am = ict_abs_mode( j.cbfMask ), s = j.signFlag ? -1 : 1;
  JccrSums       a = { 0, 0, 0, 0, 0 };
  const CrsParams crs = crs_params<CRS>( j, w, h );
  // load Cb and Cr once: the joint residual of the job's mode and its own distance
  for( int i = t; i < w * h; i += TPT )
  {
    const int  y = i / w, x = i - y * w;
    const long o = ( long ) y * j.resiStride + x;
    int        cb = cbp[o], cr = crp[o];
    crs_fwd_pair<CRS>( crs, cb, cr );
    const int  c = ict_fwd( am, s, cb, cr );
    a.fwdDist += ict_dist( am, s, cb, cr, c );
    blk[i] = c;
  }
  const int  lw = ilog2( w ), lh = ilog2( h );
  const bool ts = j.typeHor == VTMHIP_TRSKIP;
  const int  skipW = ts ? 0 : tr_skip( VTMHIP_DCT2, w ), skipH = ts ? 0 : tr_skip( VTMHIP_DCT2, h );
  chain_sync<TPT>();
  if( ts )
  {
    // xTransformSkip / xITransformSkip are plain copies: quantise the joint residual itself, without transform shift or sqrt(2) compensation
    const QuantRule qr = quant_rule_of( j, lw, lh, true );
    int            *levels = levelsBase ? levelsBase + j.outOff : nullptr;
    int16_t        *recCb = recCbBase ? recCbBase + j.outOff : nullptr, *recCr = recCrBase ? recCrBase + j.outOff : nullptr;
    for( int i = t; i < w * h; i += TPT )
    {
      const int c = blk[i];
      a.sumAbs += abs( c );
      const int q = qr.level( c, a.absSum );
      if( levels ) levels[i] = q;
      const int  y = i / w, x = i - y * w;
      const long o = ( long ) y * j.resiStride + x;
      jccr_finish<CRS>( am, s, ( int ) ( int16_t ) qr.dequant( q ), cbp[o], crp[o], recCb, recCr, i, a.sseCb, a.sseCr, crs.adj, crs.maxAbs );
    }
  }
  else
  {
    // forward: TrQuant::xT
    lds_load_matrix_T( tabs.m[lw], w, sM, t, TPT );
    chain_sync<TPT>();
    lds_fwd_pass( blk, w, tmp, h + 1, sM, w, h, ALL_LINES, w - skipW, lw + bd + 6 - 15, t, TPT, ( long long * ) nullptr );
    chain_sync<TPT>();
    lds_load_matrix_T( tabs.m[lh], h, sM, t, TPT );
    chain_sync<TPT>();
    lds_fwd_pass( tmp, h + 1, blk, w, sM, h, w, w - skipW, h - skipH, lh + 6, t, TPT, &a.sumAbs );
    chain_sync<TPT>();
    // Quant::quant + Quant::dequant, in place
    {
      const QuantRule qr = quant_rule_of( j, lw, lh, false );
      int            *levels = levelsBase ? levelsBase + j.outOff : nullptr;
      for( int i = t; i < w * h; i += TPT )
      {
        const int q = qr.level( blk[i], a.absSum );
        if( levels ) levels[i] = q;
        blk[i] = qr.dequant( q );
      }
    }
    chain_sync<TPT>();
    // inverse: TrQuant::xIT, then the inverse ICT and the two SSEs
    lds_load_matrix( tabs.m[lh], h, sM, t, TPT );
    chain_sync<TPT>();
    lds_inv_pass( blk, w, sM, h, w, w - skipW, h - skipH, 7, t, TPT, [&]( int, int i, int y, int v ) { tmp[i * h + y] = v; } );
    chain_sync<TPT>();
    lds_load_matrix( tabs.m[lw], w, sM, t, TPT );
    chain_sync<TPT>();
    int16_t *recCb = recCbBase ? recCbBase + j.outOff : nullptr, *recCr = recCrBase ? recCrBase + j.outOff : nullptr;
    lds_inv_pass( tmp, h, sM, w, h, ALL_LINES, w - skipW, 20 - bd, t, TPT, [&]( int o, int y, int x, int v ) {
      const long ro = ( long ) y * j.resiStride + x;   // the two original residuals again, from L2
      jccr_finish<CRS>( am, s, v, cbp[ro], crp[ro], recCb, recCr, o, a.sseCb, a.sseCr, crs.adj, crs.maxAbs );
    } );
  }
  jccr_reduce_store<TPT>( a, sRed, sub, t, true, results + jobIdx );
}

// ---- uniform 4x4 / 8x4 / 4x8 batches: ONE LANE per pair, the joint block in registers (tu_chain_lane_kernel between the two ICTs) ----------------------
template<int W, int H, bool CRS>
__global__ __launch_bounds__( 256 ) void jccr_chain_lane_kernel( const int16_t *__restrict__ resiBase, const vtmhip_jccr_job *__restrict__ jobs, int numJobs, DctTabs tabs,
                                                                int *__restrict__ levelsBase, int16_t *__restrict__ recCbBase, int16_t *__restrict__ recCrBase,
                                                                vtmhip_jccr_result *__restrict__ results )
{
  constexpr int LW = W == 4 ? 2 : 3, LH = H == 4 ? 2 : 3, N = W * H;
  __shared__ int16_t sMH[W * W], sMV[H * H];
  for( int i = threadIdx.x; i < W * W; i += 256 ) sMH[i] = tabs.m[LW][i];
  for( int i = threadIdx.x; i < H * H; i += 256 ) sMV[i] = tabs.m[LH][i];
  __syncthreads();
  const int jobIdx = blockIdx.x * 256 + threadIdx.x;
  if( jobIdx >= numJobs ) return;
  const vtmhip_jccr_job j = jobs[jobIdx];
  const int      bd = j.bitDepth, am = ict_abs_mode( j.cbfMask ), s = j.signFlag ? -1 : 1;
  const int16_t *cbp = resiBase + j.cbOff, *crp = resiBase + j.crOff;
  int            r[N], b[N];
  JccrSums       a = { 0, 0, 0, 0, 0 };
  const CrsParams crs = crs_params<CRS>( j, W, H );
  const bool     aligned = ( ( j.cbOff | j.crOff | j.resiStride ) & 3 ) == 0;   // 8-byte aligned rows: 4 samples per load
  if( aligned )
  {
#pragma unroll
    for( int y = 0; y < H; y++ )
#pragma unroll
      for( int x = 0; x < W; x += 4 )
      {
        const int2 vb = *reinterpret_cast<const int2 *>( cbp + ( long ) y * j.resiStride + x ), vr = *reinterpret_cast<const int2 *>( crp + ( long ) y * j.resiStride + x );
        int        cb4[4] = { ( int ) ( short ) vb.x, vb.x >> 16, ( int ) ( short ) vb.y, vb.y >> 16 }, cr4[4] = { ( int ) ( short ) vr.x, vr.x >> 16, ( int ) ( short ) vr.y, vr.y >> 16 };
#pragma unroll
        for( int q = 0; q < 4; q++ )
        {
          crs_fwd_pair<CRS>( crs, cb4[q], cr4[q] );
          const int c = ict_fwd( am, s, cb4[q], cr4[q] );
          a.fwdDist += ict_dist( am, s, cb4[q], cr4[q], c );
          r[y * W + x + q] = c;
        }
      }
  }
  else
  {
#pragma unroll
    for( int y = 0; y < H; y++ )
#pragma unroll
      for( int x = 0; x < W; x++ )
      {
        int cb = cbp[( long ) y * j.resiStride + x], cr = crp[( long ) y * j.resiStride + x];
        crs_fwd_pair<CRS>( crs, cb, cr );
        const int c = ict_fwd( am, s, cb, cr );
        a.fwdDist += ict_dist( am, s, cb, cr, c );
        r[y * W + x] = c;
      }
  }
  lane_fwd_2d<W, H>( r, b, sMH, sMV, bd, a.sumAbs );
  // Quant::quant + Quant::dequant
  {
    const QuantRule qr = quant_rule_of( j, LW, LH, false );
    int            *levels = levelsBase ? levelsBase + j.outOff : nullptr;
#pragma unroll
    for( int i = 0; i < N; i++ )
    {
      const int q = qr.level( b[i], a.absSum );
      if( levels ) levels[i] = q;
      b[i] = qr.dequant( q );
    }
  }
  // inverse; then the inverse ICT and both SSEs per sample, the original residuals read again (L2) instead of held in registers
  {
    int16_t *recCb = recCbBase ? recCbBase + j.outOff : nullptr, *recCr = recCrBase ? recCrBase + j.outOff : nullptr;
    lane_inv_2d<W, H>( b, sMH, sMV, bd, [&]( int y, int x, int v ) { r[y * W + x] = v; } );
    if( aligned )
    {
#pragma unroll
      for( int y = 0; y < H; y++ )
#pragma unroll
        for( int x = 0; x < W; x += 4 )
        {
          const int2 vb = *reinterpret_cast<const int2 *>( cbp + ( long ) y * j.resiStride + x ), vr = *reinterpret_cast<const int2 *>( crp + ( long ) y * j.resiStride + x );
          const int  cb4[4] = { ( int ) ( short ) vb.x, vb.x >> 16, ( int ) ( short ) vb.y, vb.y >> 16 }, cr4[4] = { ( int ) ( short ) vr.x, vr.x >> 16, ( int ) ( short ) vr.y, vr.y >> 16 };
#pragma unroll
          for( int q = 0; q < 4; q++ ) jccr_finish<CRS>( am, s, r[y * W + x + q], cb4[q], cr4[q], recCb, recCr, y * W + x + q, a.sseCb, a.sseCr, crs.adj, crs.maxAbs );
        }
    }
    else
    {
#pragma unroll
      for( int y = 0; y < H; y++ )
#pragma unroll
        for( int x = 0; x < W; x++ )
          jccr_finish<CRS>( am, s, r[y * W + x], cbp[( long ) y * j.resiStride + x], crp[( long ) y * j.resiStride + x], recCb, recCr, y * W + x, a.sseCb, a.sseCr, crs.adj,
                            crs.maxAbs );
    }
  }
  results[jobIdx] = jccr_result_of( a );
}

// ---- uniform batches with power-of-two sides >= 8: tu_stages.hpp's register-blocked passes (a lane owns a 2 x 8 block of outputs), as tu_chain_uni_kernel ----
template<int LPT, bool CRS>
__global__ __launch_bounds__( 256 ) void jccr_chain_uni_kernel( const int16_t *__restrict__ resiBase, const vtmhip_jccr_job *__restrict__ jobs, int numJobs, DctTabs tabs,
                                                               int *__restrict__ levelsBase, int16_t *__restrict__ recCbBase, int16_t *__restrict__ recCrBase,
                                                               vtmhip_jccr_result *__restrict__ results, int w, int h )
{
  extern __shared__ __attribute__( ( aligned( 16 ) ) ) int ldsw[];
  __shared__ long long sRed[4][5];
  constexpr int TUS = 256 / LPT;
  const int     sub = threadIdx.x / LPT, t = threadIdx.x - sub * LPT;
  const int     perTu = w * h + w * ( h + 1 );   // ints: blk, tmp (the 16-bit joint residual lives in blk until the second forward pass overwrites it)
  int16_t      *sMat = ( int16_t * ) ( ldsw + TUS * perTu );
  const int     lw = ilog2( w ), lh = ilog2( h );
  // width:  mW0 = M_W with rows k, k+1 interleaved (second inverse pass), mW1 = M_W^T with rows n, n+1 interleaved (first forward pass)
  // height: mH0 = M_H with rows k, k+1 interleaved (first inverse pass),   mH1 = M_H^T plain (second forward pass: 32-bit input)
  int16_t *mW0 = sMat, *mW1 = mW0 + w * w, *mH0 = mW1 + w * w, *mH1 = mH0 + h * h;
  tuq_stage_matrix<false>( tabs.m[lw], w, lw, mW0, mW1 );
  tuq_stage_matrix<true>( tabs.m[lh], h, lh, mH0, mH1 );
  __syncthreads();
  const int  jobIdx = blockIdx.x * TUS + sub;
  const bool live   = jobIdx < numJobs;   // dead groups (whole waves or idle lane groups) compute the last job again and write nothing: they only meet the barriers
  const vtmhip_jccr_job j = jobs[live ? jobIdx : numJobs - 1];
  const int      bd = j.bitDepth, am = ict_abs_mode( j.cbfMask ), s = j.signFlag ? -1 : 1;
  int           *blk = ldsw + sub * perTu, *tmp = blk + w * h;
  int16_t       *sR  = ( int16_t * ) blk;
  const int16_t *cbp = resiBase + j.cbOff, *crp = resiBase + j.crOff;
  JccrSums       a = { 0, 0, 0, 0, 0 };
  const CrsParams crs = crs_params<CRS>( j, w, h );
  for( int i = t; i < w * h; i += LPT )
  {
    const long o  = ( long ) ( i >> lw ) * j.resiStride + ( i & ( w - 1 ) );
    int        cb = cbp[o], cr = crp[o];
    crs_fwd_pair<CRS>( crs, cb, cr );
    const int  c = ict_fwd( am, s, cb, cr );
    a.fwdDist += ict_dist( am, s, cb, cr, c );
    sR[i] = ( int16_t ) c;
  }
  int16_t *dq16 = reinterpret_cast<int16_t *>( tmp );   // dequantised coefficients [k][k2] (after the second forward pass has consumed tmp)
  int16_t *t16  = reinterpret_cast<int16_t *>( blk );   // first inverse pass output [y][i] (after quantisation has consumed blk)
  int     *rec32 = tmp;                                  // reconstructed joint residual [y][x]
  const int skipW = tr_skip( VTMHIP_DCT2, w ), skipH = tr_skip( VTMHIP_DCT2, h );
  chain_sync<LPT>();
  // forward (TrQuant::xT): tmp[k][y] = sum_n sR[y][n] * MT_hor[n][k];  blk[k2][j2] = sum_n tmp[j2][n] * MT_ver[n][k2]
  tuq_pass16<LPT, false>( sR, w, reinterpret_cast<const unsigned *>( mW1 ), w, h, w, h, w - skipW, tmp, 1, h + 1, lw + bd + 6 - 15, t );
  chain_sync<LPT>();
  tuq_pass<LPT, false>( tmp, h + 1, 1, mH1, h, h, w, h, w - skipW, h - skipH, blk, 1, w, lh + 6, t, &a.sumAbs );
  chain_sync<LPT>();
  {
    const QuantRule qr = quant_rule_of( j, lw, lh, false );
    int            *levels = ( levelsBase && live ) ? levelsBase + j.outOff : nullptr;
    for( int i = t; i < w * h; i += LPT )
    {
      const int q = qr.level( blk[i], a.absSum );
      if( levels ) levels[i] = q;
      dq16[( ( i & ( w - 1 ) ) << lh ) + ( i >> lw )] = ( int16_t ) qr.dequant( q );   // transposed: the vertical index contiguous
    }
  }
  chain_sync<LPT>();
  // inverse (TrQuant::xIT): t16[y][i] = clip( sum_k dq[k][i] * M_ver[k][y] );  rec[y][x] = clip( sum_k t16[y][k] * M_hor[k][x] )
  tuq_pass16<LPT, true>( dq16, h, reinterpret_cast<const unsigned *>( mH0 ), h - skipH, w, h, w - skipW, h, t16, 1, w, 7, t );
  chain_sync<LPT>();
  tuq_pass16<LPT, true>( t16, w, reinterpret_cast<const unsigned *>( mW0 ), w - skipW, h, w, h, w, rec32, w, 1, 20 - bd, t );
  chain_sync<LPT>();
  {
    int16_t *recCb = ( recCbBase && live ) ? recCbBase + j.outOff : nullptr, *recCr = ( recCrBase && live ) ? recCrBase + j.outOff : nullptr;
    for( int i = t; i < w * h; i += LPT )
    {
      const long o = ( long ) ( i >> lw ) * j.resiStride + ( i & ( w - 1 ) );   // the two original residuals again, from L2
      jccr_finish<CRS>( am, s, rec32[i], cbp[o], crp[o], recCb, recCr, i, a.sseCb, a.sseCr, crs.adj, crs.maxAbs );
    }
  }
  jccr_reduce_store<LPT>( a, sRed, sub, t, live, results + ( live ? jobIdx : 0 ) );
}

DctTabs tabs_of( const vtmhip_ctx *ctx )
{
  DctTabs t;
  for( int l = 0; l < 7; l++ ) t.m[l] = ctx->trTab[VTMHIP_DCT2][l];
  return t;
}

bool pow2( int v ) { return v > 0 && ( v & ( v - 1 ) ) == 0; }

template<int W, int H, bool CRS>
int launch_lane( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_jccr_job *d_jobs, int n, int32_t *d_levelsBase, int16_t *d_recCbBase, int16_t *d_recCrBase,
                 vtmhip_jccr_result *d_results )
{
  VTMHIP_TIME_KERNEL( ctx, "jccr_chain_lane_kernel" );
  hipLaunchKernelGGL( ( jccr_chain_lane_kernel<W, H, CRS> ), dim3( ( n + 255 ) / 256 ), dim3( 256 ), 0, ctx->stream, d_resiBase, d_jobs, n, tabs_of( ctx ), d_levelsBase,
                      d_recCbBase, d_recCrBase, d_results );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

template<int LPT, bool CRS>
int launch_uni( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_jccr_job *d_jobs, int n, int w, int h, int32_t *d_levelsBase, int16_t *d_recCbBase,
                int16_t *d_recCrBase, vtmhip_jccr_result *d_results )
{
  constexpr int TUS = 256 / LPT;
  const size_t  lds = TUS * ( ( size_t ) w * h + ( size_t ) w * ( h + 1 ) ) * sizeof( int ) + ( 2 * ( size_t ) w * w + 2 * ( size_t ) h * h ) * sizeof( int16_t );
  if( lds > 64 * 1024 )   // 64x64 only: 64.3 KB
    VTMHIP_HIP( ctx, hipFuncSetAttribute( reinterpret_cast<const void *>( jccr_chain_uni_kernel<LPT, CRS> ), hipFuncAttributeMaxDynamicSharedMemorySize, ( int ) lds ) );
  VTMHIP_TIME_KERNEL( ctx, "jccr_chain_uni_kernel" );
  hipLaunchKernelGGL( ( jccr_chain_uni_kernel<LPT, CRS> ), dim3( ( n + TUS - 1 ) / TUS ), dim3( 256 ), lds, ctx->stream, d_resiBase, d_jobs, n, tabs_of( ctx ), d_levelsBase,
                      d_recCbBase, d_recCrBase, d_results, w, h );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

// vtmhip_jccr_chain_batch_dev (CRS == false) and vtmhip_jccr_chain_crs_batch_dev: the host check of the job table (jccr_chain_entry), then one dispatch with the
// same launch paths (jccr_chain_dispatch: it launches and nothing else, for a caller whose jobs are checked already)
template<bool CRS>
int jccr_chain_dispatch( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_jccr_job *d_jobs, int n, int maxWidth, int maxHeight, int uniformSize,
                         int32_t *d_levelsBase, int16_t *d_recCbBase, int16_t *d_recCrBase, vtmhip_jccr_result *d_results );

template<bool CRS>
int jccr_chain_entry( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_jccr_job *d_jobs, int n, int maxWidth, int maxHeight, int uniformSize,
                      int32_t *d_levelsBase, int16_t *d_recCbBase, int16_t *d_recCrBase, vtmhip_jccr_result *d_results )
{
  VTMHIP_BATCH_ENTRY( ctx, n, d_resiBase && d_jobs && d_results );
  VTMHIP_REQUIRE( ctx, maxWidth >= 2 && maxWidth <= 64 && maxHeight >= 2 && maxHeight <= 64, "maxWidth / maxHeight: 2..64 (2-D transforms)" );
  const bool uniPath = uniformSize && maxWidth >= 8 && maxHeight >= 8;
  if( uniPath ) VTMHIP_REQUIRE( ctx, pow2( maxWidth ) && pow2( maxHeight ), "uniformSize: width / height must be powers of two (TU sizes are)" );
  int st = vtmhip_internal_tr_tables( ctx );
  if( st ) return st;
  // the job table, checked on the host before anything is launched (the kernels index LDS and the core matrices by these fields)
  {
    HostStage              hs( ctx );
    const vtmhip_jccr_job *jobs = nullptr;
    VTMHIP_TRY( hs.pull_table( d_jobs, n, jobs ) );
    for( int i = 0; i < n; i++ )
    {
      const vtmhip_jccr_job &j = jobs[i];
      const bool ts = j.typeHor == VTMHIP_TRSKIP;
      VTMHIP_REQUIRE( ctx, j.cbfMask >= 1 && j.cbfMask <= 3, "cbfMask: 1 .. 3" );
      VTMHIP_REQUIRE( ctx, ts || j.typeHor == VTMHIP_DCT2, "typeHor: VTMHIP_DCT2 or VTMHIP_TRSKIP" );
      VTMHIP_REQUIRE( ctx, pow2( j.width ) && pow2( j.height ) && j.width >= 2 && j.height >= 2 && j.width <= maxWidth && j.height <= maxHeight,
                      "width / height: powers of two, 2 .. maxWidth / maxHeight" );
      VTMHIP_REQUIRE( ctx, !ts || ( j.width <= 32 && j.height <= 32 ), "transform skip: sides <= 32 (log2MaxTransformSkipBlockSize)" );
      VTMHIP_REQUIRE( ctx, j.bitDepth >= 8 && j.bitDepth <= 12 && j.qpRem >= 0 && j.qpRem < 6 && j.qpPer >= 0, "bitDepth 8..12, qpRem 0..5, qpPer >= 0" );
      VTMHIP_REQUIRE( ctx, !CRS || j.chromaAdj <= 32767, "chromaAdj: 0 (no scaling) .. 32767" );
      VTMHIP_REQUIRE( ctx, !uniformSize || ( !ts && j.width == maxWidth && j.height == maxHeight ), "uniformSize: every job maxWidth x maxHeight with VTMHIP_DCT2" );
    }
  }
  return jccr_chain_dispatch<CRS>( ctx, d_resiBase, d_jobs, n, maxWidth, maxHeight, uniformSize, d_levelsBase, d_recCbBase, d_recCrBase, d_results );
}

template<bool CRS>
int jccr_chain_dispatch( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_jccr_job *d_jobs, int n, int maxWidth, int maxHeight, int uniformSize,
                         int32_t *d_levelsBase, int16_t *d_recCbBase, int16_t *d_recCrBase, vtmhip_jccr_result *d_results )
{
  const bool lanePath = uniformSize && maxWidth * maxHeight <= 32 && maxWidth >= 4 && maxHeight >= 4;
  const bool uniPath  = uniformSize && maxWidth >= 8 && maxHeight >= 8;
  if( lanePath )
  {
    if( maxWidth == 4 && maxHeight == 4 ) return launch_lane<4, 4, CRS>( ctx, d_resiBase, d_jobs, n, d_levelsBase, d_recCbBase, d_recCrBase, d_results );
    if( maxWidth == 8 ) return launch_lane<8, 4, CRS>( ctx, d_resiBase, d_jobs, n, d_levelsBase, d_recCbBase, d_recCrBase, d_results );
    return launch_lane<4, 8, CRS>( ctx, d_resiBase, d_jobs, n, d_levelsBase, d_recCbBase, d_recCrBase, d_results );
  }
  if( uniPath )
  {
    const int items = maxWidth * maxHeight / 16;   // one lane = 2 x 8 outputs of a transform pass
#define VTMHIP_JCCR_UNI( LPT ) launch_uni<LPT, CRS>( ctx, d_resiBase, d_jobs, n, maxWidth, maxHeight, d_levelsBase, d_recCbBase, d_recCrBase, d_results )
    if( items <= 4 ) return VTMHIP_JCCR_UNI( 4 );
    if( items <= 8 ) return VTMHIP_JCCR_UNI( 8 );
    if( items <= 16 ) return VTMHIP_JCCR_UNI( 16 );
    if( items <= 32 ) return VTMHIP_JCCR_UNI( 32 );
    if( items <= 64 ) return VTMHIP_JCCR_UNI( 64 );
    if( items <= 128 ) return VTMHIP_JCCR_UNI( 128 );
    return VTMHIP_JCCR_UNI( 256 );
#undef VTMHIP_JCCR_UNI
  }
  const int    mx    = maxWidth > maxHeight ? maxWidth : maxHeight;
  const size_t perTu = ( size_t ) maxWidth * maxHeight + ( size_t ) maxWidth * ( maxHeight + 1 ) + ( ( mx * mx + 1 ) >> 1 );
  VTMHIP_TIME_KERNEL( ctx, "jccr_chain_kernel" );
  if( maxWidth * maxHeight <= 256 )
    hipLaunchKernelGGL( ( jccr_chain_kernel<64, CRS> ), dim3( ( n + 3 ) / 4 ), dim3( 256 ), 4 * perTu * sizeof( int ), ctx->stream, d_resiBase, d_jobs, n, tabs_of( ctx ), d_levelsBase,
                        d_recCbBase, d_recCrBase, d_results, maxWidth, maxHeight );
  else
    hipLaunchKernelGGL( ( jccr_chain_kernel<256, CRS> ), dim3( n ), dim3( 256 ), perTu * sizeof( int ), ctx->stream, d_resiBase, d_jobs, n, tabs_of( ctx ), d_levelsBase, d_recCbBase,
                        d_recCrBase, d_results, maxWidth, maxHeight );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

}   // namespace

extern "C"
{

int vtmhip_jccr_struct_size( int which )
{
  switch( which )
  {
  case 0: return ( int ) sizeof( vtmhip_ict_job );
  case 1: return ( int ) sizeof( vtmhip_jccr_job );
  case 2: return ( int ) sizeof( vtmhip_jccr_result );
  default: return -1;
  }
}

int vtmhip_fwdTransformCbCr( vtmhip_ctx *ctx, int mode, const int16_t *cb, int cbStride, const int16_t *cr, int crStride, int16_t *c1, int c1Stride, int16_t *c2,
                             int c2Stride, int width, int height, int64_t dist[2] )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, mode >= -3 && mode <= 3, "mode: -3 .. 3 (m_fwdICT has seven slots)" );
  VTMHIP_REQUIRE( ctx, width >= 1 && width <= 64 && height >= 1 && height <= 64, "width / height: 1 .. 64" );
  const int am = mode < 0 ? -mode : mode, cbfMask = am == 3 ? 1 : am == 0 ? 0 : am + 1;
  int16_t  *joint = am == 3 ? c2 : c1;
  const int jointStride = am == 3 ? c2Stride : c1Stride;
  VTMHIP_REQUIRE( ctx, cb && cr && dist && ( am == 0 || joint ), "null pointer" );
  HostStage    s( ctx );
  const size_t blk = ( size_t ) width * height * sizeof( int16_t );
  const size_t cbOff = s.region( blk ), crOff = s.region( blk ), jointOff = s.region( blk ), jobOff = s.region( sizeof( vtmhip_ict_job ) ), outOff = s.region( 64 );   // dist[4][2]
  VTMHIP_TRY( s.reserve() );
  s.pack( cbOff, cb, cbStride, width, height );
  s.pack( crOff, cr, crStride, width, height );
  vtmhip_ict_job j;
  memset( &j, 0, sizeof( j ) );
  j.cbOff = ( int64_t ) ( cbOff / 2 ); j.crOff = ( int64_t ) ( crOff / 2 ); j.cbStride = j.crStride = width;
  j.outOff = ( int64_t ) ( jointOff / 2 ) - ( int64_t ) ( cbfMask ? cbfMask - 1 : 0 ) * width * height;   // the requested plane lands in the joint region
  j.width = ( int16_t ) width; j.height = ( int16_t ) height; j.signFlag = mode < 0; j.maskBits = ( uint8_t ) ( cbfMask ? 1 << cbfMask : 0 );
  s.put( jobOff, j );
  VTMHIP_TRY( s.upload( 0, outOff ) );
  hipLaunchKernelGGL( ict_fwd_kernel, dim3( 1 ), dim3( 256 ), 0, ctx->stream, s.dev<const int16_t>( 0 ), s.dev<const vtmhip_ict_job>( jobOff ), 1, s.dev<int16_t>( 0 ),
                      s.dev<long long>( outOff ) );
  VTMHIP_LAUNCHED( ctx );
  VTMHIP_TRY( s.download( jointOff, blk ) );
  VTMHIP_TRY( s.fetch( outOff, 64 ) );
  memcpy( dist, s.hp + outOff + 16 * cbfMask, 16 );
  if( am ) s.unpack( joint, jointStride, jointOff, width, height );
  return VTMHIP_OK;
}

int vtmhip_invTransformCbCr( vtmhip_ctx *ctx, int mode, int16_t *cb, int cbStride, int16_t *cr, int crStride, int width, int height )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, mode >= -3 && mode <= 3, "mode: -3 .. 3 (m_invICT has seven slots)" );
  VTMHIP_REQUIRE( ctx, width >= 1 && width <= 64 && height >= 1 && height <= 64, "width / height: 1 .. 64" );
  VTMHIP_REQUIRE( ctx, cb && cr, "null pointer" );
  if( mode == 0 ) return VTMHIP_OK;   // invTransformCbCr<0> touches nothing
  HostStage    s( ctx );
  const size_t blk = ( size_t ) width * height * sizeof( int16_t ), cbOff = s.region( blk ), crOff = s.region( blk );
  VTMHIP_TRY( s.reserve() );
  s.pack( cbOff, cb, cbStride, width, height );
  s.pack( crOff, cr, crStride, width, height );
  VTMHIP_TRY( s.upload( 0, s.total ) );
  const int count = width * height;
  hipLaunchKernelGGL( ict_inv_kernel, dim3( ( count + 255 ) / 256 ), dim3( 256 ), 0, ctx->stream, s.dev<int16_t>( cbOff ), s.dev<int16_t>( crOff ), count,
                      mode < 0 ? -mode : mode, mode < 0 ? -1 : 1 );
  VTMHIP_LAUNCHED( ctx );
  VTMHIP_TRY( s.fetch( 0, s.total ) );
  if( mode == 3 || mode == -3 ) s.unpack( cb, cbStride, cbOff, width, height );
  else s.unpack( cr, crStride, crOff, width, height );
  return VTMHIP_OK;
}

int vtmhip_ict_fwd_batch_dev( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_ict_job *d_jobs, int n, int16_t *d_jointBase, int64_t *d_dist )
{
  VTMHIP_BATCH_ENTRY( ctx, n, d_resiBase && d_jobs && d_dist );
  VTMHIP_TIME_KERNEL( ctx, "ict_fwd_kernel" );
  hipLaunchKernelGGL( ict_fwd_kernel, dim3( ( n + 3 ) / 4 ), dim3( 256 ), 0, ctx->stream, d_resiBase, d_jobs, n, d_jointBase, ( long long * ) d_dist );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

int vtmhip_ict_select( const int64_t dist[4][2], int isIntra, int masks[2], int *numMasks )
{
  if( !dist || !masks || !numMasks ) return VTMHIP_E_INVALID;
  *numMasks = 0;
  if( !isIntra ) { masks[( *numMasks )++] = 3; return VTMHIP_OK; }
  int64_t minDist1 = dist[0][0] < dist[0][1] ? dist[0][0] : dist[0][1], minDist2 = INT64_MAX;
  int     cbfMask1 = 0, cbfMask2 = 0;
  for( int cbfMask = 1; cbfMask <= 3; cbfMask++ )
  {
    if( dist[cbfMask][0] < minDist1 )
    {
      cbfMask2 = cbfMask1; minDist2 = minDist1;
      cbfMask1 = cbfMask;  minDist1 = dist[cbfMask1][0];
    }
    else if( dist[cbfMask][0] < minDist2 )
    {
      cbfMask2 = cbfMask; minDist2 = dist[cbfMask2][0];
    }
  }
  if( cbfMask1 ) masks[( *numMasks )++] = cbfMask1;
  if( cbfMask2 && ( ( minDist2 < ( 9 * minDist1 ) / 8 ) || ( !cbfMask1 && minDist2 < ( 3 * minDist1 ) / 2 ) ) ) masks[( *numMasks )++] = cbfMask2;
  return VTMHIP_OK;
}

int vtmhip_jccr_chain_batch_dev( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_jccr_job *d_jobs, int n, int maxWidth, int maxHeight, int uniformSize,
                                 int32_t *d_levelsBase, int16_t *d_recCbBase, int16_t *d_recCrBase, vtmhip_jccr_result *d_results )
{
  return jccr_chain_entry<false>( ctx, d_resiBase, d_jobs, n, maxWidth, maxHeight, uniformSize, d_levelsBase, d_recCbBase, d_recCrBase, d_results );
}

int vtmhip_jccr_chain_crs_batch_dev( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_jccr_job *d_jobs, int n, int maxWidth, int maxHeight, int uniformSize,
                                     int32_t *d_levelsBase, int16_t *d_recCbBase, int16_t *d_recCrBase, vtmhip_jccr_result *d_results )
{
  return jccr_chain_entry<true>( ctx, d_resiBase, d_jobs, n, maxWidth, maxHeight, uniformSize, d_levelsBase, d_recCbBase, d_recCrBase, d_results );
}

}   // extern "C"

// the dispatch of vtmhip_jccr_chain_batch_dev (crs: of vtmhip_jccr_chain_crs_batch_dev) without the read-back of the job table, for intra_chroma_chain.hip: its jobs
// are expanded on the device from tables the entry has checked (power-of-two sides 4 .. 32, cbfMask 1 .. 3, DCT2 or transform skip, uniformSize as found).
// It stands behind the public entries and names the plain instantiation first: the order of first use is the order of the kernels in the object.
int vtmhip_internal_jccr_chain_launch( vtmhip_ctx *ctx, bool crs, const int16_t *d_resiBase, const vtmhip_jccr_job *d_jobs, int n, int maxWidth, int maxHeight,
                                       int uniformSize, int32_t *d_levelsBase, int16_t *d_recCbBase, int16_t *d_recCrBase, vtmhip_jccr_result *d_results )
{
  VTMHIP_TRY( vtmhip_internal_tr_tables( ctx ) );
  if( !crs ) return jccr_chain_dispatch<false>( ctx, d_resiBase, d_jobs, n, maxWidth, maxHeight, uniformSize, d_levelsBase, d_recCbBase, d_recCrBase, d_results );
  return jccr_chain_dispatch<true>( ctx, d_resiBase, d_jobs, n, maxWidth, maxHeight, uniformSize, d_levelsBase, d_recCbBase, d_recCrBase, d_results );
}
