// tu_stages.hpp -- the stages of the fused residual chain (xT -> Quant::quant -> Quant::dequant -> xIT), defined once for every kernel that runs them:
// the single-component chain of transform.hip (tu_chain_kernel / tu_chain_lane_kernel / tu_chain_uni_kernel / tu_ts_kernel, quant_kernel, dequant_kernel,
// xT_kernel, xIT_kernel) and the joint Cb-Cr chain of jccr.hip (jccr_chain_kernel / jccr_chain_lane_kernel / jccr_chain_uni_kernel).  The kernels keep their
// loads, LDS layouts and epilogues; what a stage computes, and in which order of the integer operations, is written here only.
//
// Reference: TrQuant::xT CommonLib/TrQuant.cpp:776-851, xIT :853-923 (the "fast" butterflies of TrQuant_EMT.cpp are exact refactorings of the matrix product,
// so a plain 32-bit integer product is bit-identical, wrap-around included); Quant::quant CommonLib/Quant.cpp:955-1038, Quant::dequant :357-482 (flat scaling
// list), g_quantScales / g_invQuantScales CommonLib/Rom.cpp:463-473.
#pragma once
#include "ctx.hpp"

namespace
{

__device__ __forceinline__ int ilog2( int v ) { return 31 - __clz( v ); }
__device__ __forceinline__ int clip16( int v ) { return min( 32767, max( -32768, v ) ); }

// zero-out: the last tr_skip( type, n ) of the n frequencies of a dimension are not computed (TrQuant.cpp:792-796): DST-7 / DCT-8 keep 16 of 32, DCT-2 32 of 64
__device__ __forceinline__ int tr_skip( int type, int n ) { return ( type != VTMHIP_DCT2 && n == 32 ) ? 16 : ( n > 32 ? n - 32 : 0 ); }

// ---- 1. scalar quantisation, flat scaling list ------------------------------------------------------------------------------------------------------------
__constant__ int c_quantScales[2][6]    = { { 26214, 23302, 20560, 18396, 16384, 14564 }, { 18396, 16384, 14564, 13107, 11651, 10280 } };   // [needSqrt][qpRem]
__constant__ int c_invQuantScales[2][6] = { { 40, 45, 51, 57, 64, 72 }, { 57, 64, 72, 80, 90, 102 } };

// The rule of one TU.  Transform skip (xTransformSkip / xITransformSkip are plain copies, TrQuant.cpp:1200-1213, 925-941) knows neither the transform shift nor
// the sqrt(2) compensation of blocks with an odd log2 w + log2 h; its caller puts QpParam::per( true ) / rem( true ) into the job.
struct QuantRule
{
  long long add;
  int       qBits, scale;                       // Quant::quant
  int       iscale, rightShift, inMin, inMax;   // Quant::dequant

  // |c| * scale and the magnitude of the level; quant_kernel derives its deltaU from the two
  __device__ __forceinline__ int mag( int c, long long &scaled ) const
  {
    scaled = ( long long ) abs( c ) * scale;
    return ( int ) ( ( scaled + add ) >> qBits );
  }

  __device__ __forceinline__ int signed_level( int c, int m ) const { return clip16( c < 0 ? -m : m ); }

  template<class SumT>
  __device__ __forceinline__ int level( int c, SumT &absSum ) const
  {
    long long scaled;
    const int m = mag( c, scaled );
    absSum += m;
    return signed_level( c, m );
  }

  __device__ __forceinline__ int dequant( int q ) const
  {
    const int qq = min( inMax, max( inMin, q ) );
    int       v;
    if( rightShift > 0 ) v = ( int ) ( ( unsigned ) ( qq * iscale ) + ( 1u << ( rightShift - 1 ) ) ) >> rightShift;
    else v = ( int ) ( ( unsigned ) ( qq * iscale ) << ( -rightShift ) );
    return clip16( v );
  }
};

// lw, lh: log2 of the TU's sides (constants in the one-lane kernels: needSqrt folds)
__device__ __forceinline__ QuantRule quant_rule( int bitDepth, int qpPer, int qpRem, int isIRAP, int lw, int lh, bool transformSkip )
{
  const int needSqrt = transformSkip ? 0 : ( lw + lh ) & 1;
  const int trShift  = transformSkip ? 0 : 15 - bitDepth - ( ( lw + lh ) >> 1 ) + ( needSqrt ? -1 : 0 );
  QuantRule p;
  p.qBits      = 14 + qpPer + trShift;
  p.add        = ( long long ) ( isIRAP ? 171 : 85 ) << ( p.qBits - 9 );
  p.scale      = c_quantScales[needSqrt][qpRem];
  p.iscale     = c_invQuantScales[needSqrt][qpRem];
  p.rightShift = 6 - ( trShift + qpPer );
  const int inBits = min( 16, 32 + p.rightShift - 7 );
  p.inMin = -( 1 << ( inBits - 1 ) );
  p.inMax = ( 1 << ( inBits - 1 ) ) - 1;
  return p;
}

// ---- 2. synchronisation and reduction of a group of LANES lanes that share one TU -------------------------------------------------------------------------------
// LANES <= 64: the group lies inside one wave (wave-level synchronisation only); above: the whole workgroup
template<int LANES>
__device__ __forceinline__ void chain_sync()
{
  if( LANES <= 64 ) { __builtin_amdgcn_fence( __ATOMIC_ACQ_REL, "wavefront" ); __builtin_amdgcn_wave_barrier(); }
  else __syncthreads();
}

// chain_sync that also votes: true when NO lane raised `flag`.  The vote is taken over everything that would have to take the other path together -- the whole
// wave for LANES <= 64 (a lane group that left the work alone inside a busy wave saves nothing), the whole workgroup above (__syncthreads_or is the barrier, so
// both paths meet the same number of them) -- and is therefore uniform over the wave / workgroup.  The chains decide "no level of these TUs is non-zero" with
// it: a lane raises its flag when its partial sum of |level| is not zero (the partials are non-negative, so all partials zero <=> all levels zero); the lanes
// of dead groups never raise it.
template<int LANES>
__device__ __forceinline__ bool chain_sync_none( bool flag )
{
  if( LANES <= 64 )
  {
    const bool none = __ballot( flag ) == 0;
    chain_sync<LANES>();
    return none;
  }
  return !__syncthreads_or( flag );
}

// K sums over the group: xor-shuffles inside a wave, across the LANES / 64 waves of the group through sRed ([waves of the workgroup][K]; unused, may be null, for
// LANES <= 64).  Lane t == 0 of a live group then calls store( totals ), which packs them into the kernel's result struct.  Every lane of the workgroup must
// arrive (LANES > 64 meets at barriers).
template<int LANES, int K, class Store>
__device__ __forceinline__ void chain_reduce_store( long long ( &v )[K], long long ( *sRed )[K], int sub, int t, bool live, Store store )
{
  if( LANES <= 64 )
  {
#pragma unroll
    for( int o = 32; o > 0; o >>= 1 )
      if( o < LANES )
      {
#pragma unroll
        for( int k = 0; k < K; k++ ) v[k] += __shfl_xor( v[k], o, 64 );
      }
    if( t == 0 && live ) store( v );
    return;
  }
#pragma unroll
  for( int k = 0; k < K; k++ ) v[k] = ( long long ) wave_reduce_add_u64( ( unsigned long long ) v[k] );
  __syncthreads();
  if( ( threadIdx.x & 63 ) == 0 )
  {
#pragma unroll
    for( int k = 0; k < K; k++ ) sRed[threadIdx.x >> 6][k] = v[k];
  }
  __syncthreads();
  constexpr int WPT = LANES > 64 ? LANES / 64 : 1;   // waves per TU
  if( t == 0 && live )
  {
    long long r[K];
#pragma unroll
    for( int k = 0; k < K; k++ ) r[k] = 0;
    for( int q = 0; q < WPT; q++ )
#pragma unroll
      for( int k = 0; k < K; k++ ) r[k] += sRed[sub * WPT + q][k];
    store( r );
  }
}

// ---- 3. register-blocked passes (batches of one TU size, sides >= 8) --------------------------------------------------------------------------------------------
// Every pass is out[r][c] = sum_n A(r, n) * B[n][c] with B = the core matrix in the orientation that makes B[n][c .. c+7] contiguous (forward: transposed,
// inverse: plain).  A lane owns a 2 x 8 block of outputs (rows r, r + 1): the 16-byte matrix read of a summation step feeds 16 multiply-adds (one LDS read per
// multiply-add would leave the kernel LDS-issue bound).  rows x cols outputs (cols multiple of 8, a power of two as TU sizes are); rEff / cEff: outputs beyond
// them are zero (zero-out); inner: summation length; t, LPT: the lane's index in its group and the group's size.
//
// Headroom.  Matrix entries are |m| <= 91.  The packed passes (tuq_pass16) take int16 A values -- residuals, joint residuals (a Pel: the whole int16 range),
// dequantised coefficients and the first inverse pass's output, both clipped to 16 bits: v_dot2 of int16 pairs into a 32-bit accumulator is exact for |sum| <=
// N * 32768 * 91 < 2^31 (N <= 64).  The 24-bit multiplies of the second forward pass (tuq_pass / tuq_pass_il; v_mad_i32_i24 issues at full rate, v_mul_lo_u32 at
// a quarter of it) need |A| < 2^23: the first forward pass of int16 input is bounded by sum|m| * 32768 >> (log2 N + bitDepth - 9) <= 64 N * 2^15 >> (log2 N +
// bitDepth - 9) = 2^(30 - bitDepth) <= 2^22 for bitDepth >= 8.  The bound is the joint chain's; the residuals of one component stay at 2^bitDepth - 1 (LMCS
// fwd() clips to it), joint ones at 6 (2^bitDepth - 1) / 5.
template<int LPT, bool CLIP>
__device__ __forceinline__ void tuq_pass( const int *A, int aRowStride, int aColStride, const int16_t *B, int ldb, int inner, int rows, int cols,
                                          int rEff, int cEff, int *out, int oRowStride, int oColStride, int shift, int t, long long *sumAbs )
{
  const int cb = cols >> 3, lcb = 31 - __clz( cb ), rnd = shift > 0 ? 1 << ( shift - 1 ) : 0;
  for( int it = t; it < ( rows >> 1 ) * cb; it += LPT )
  {
    const int r = ( it >> lcb ) << 1, c0 = ( it & ( cb - 1 ) ) << 3;
    int       acc[2][8];
#pragma unroll
    for( int i = 0; i < 8; i++ ) acc[0][i] = acc[1][i] = rnd;
    if( r < rEff && c0 < cEff )
    {
      const int *a0 = A + r * aRowStride, *a1 = a0 + aRowStride;
      for( int n = 0; n < inner; n++ )
      {
        const int  av0 = a0[n * aColStride], av1 = a1[n * aColStride];
        const int4 bv = *reinterpret_cast<const int4 *>( B + n * ldb + c0 );
        const int  b[8] = { ( int ) ( short ) bv.x, bv.x >> 16, ( int ) ( short ) bv.y, bv.y >> 16, ( int ) ( short ) bv.z, bv.z >> 16, ( int ) ( short ) bv.w, bv.w >> 16 };
#pragma unroll
        for( int i = 0; i < 8; i++ ) { acc[0][i] += __mul24( av0, b[i] ); acc[1][i] += __mul24( av1, b[i] ); }
      }
    }
#pragma unroll
    for( int q = 0; q < 2; q++ )
#pragma unroll
      for( int i = 0; i < 8; i++ )
      {
        int v = ( r + q < rEff && c0 + i < cEff ) ? acc[q][i] >> shift : 0;
        if( CLIP ) v = clip16( v );
        out[( r + q ) * oRowStride + ( c0 + i ) * oColStride] = v;
        if( sumAbs ) *sumAbs += abs( v );
      }
  }
}

// tuq_pass with the matrix in the pair-interleaved layout of tuq_pass16 (Bp[(n >> 1) * cols + c] = (B[n][c], B[n+1][c])): square TUs take the second
// forward pass's M^T from the slot the first one uses, so no plain copy is staged.  Two summation steps per trip; same loads per step as tuq_pass.
template<int LPT, bool CLIP>
__device__ __forceinline__ void tuq_pass_il( const int *A, int aRowStride, int aColStride, const unsigned *Bp, int inner, int rows, int cols, int rEff, int cEff,
                                             int *out, int oRowStride, int oColStride, int shift, int t, long long *sumAbs )
{
  const int cb = cols >> 3, lcb = 31 - __clz( cb ), rnd = shift > 0 ? 1 << ( shift - 1 ) : 0;
  for( int it = t; it < ( rows >> 1 ) * cb; it += LPT )
  {
    const int r = ( it >> lcb ) << 1, c0 = ( it & ( cb - 1 ) ) << 3;
    int       acc[2][8];
#pragma unroll
    for( int i = 0; i < 8; i++ ) acc[0][i] = acc[1][i] = rnd;
    if( r < rEff && c0 < cEff )
    {
      const int *a0 = A + r * aRowStride, *a1 = a0 + aRowStride;
      for( int n2 = 0; n2 < ( inner >> 1 ); n2++ )
      {
        const int   n = n2 << 1;
        const int   e0 = a0[n * aColStride], o0 = a0[( n + 1 ) * aColStride], e1 = a1[n * aColStride], o1 = a1[( n + 1 ) * aColStride];
        const uint4 b0 = *reinterpret_cast<const uint4 *>( Bp + n2 * cols + c0 ), b1 = *reinterpret_cast<const uint4 *>( Bp + n2 * cols + c0 + 4 );
        const unsigned bw[8] = { b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w };
#pragma unroll
        for( int i = 0; i < 8; i++ )
        {
          const int be = ( int ) ( short ) bw[i], bo = ( int ) bw[i] >> 16;
          acc[0][i] += __mul24( e0, be ) + __mul24( o0, bo );
          acc[1][i] += __mul24( e1, be ) + __mul24( o1, bo );
        }
      }
    }
#pragma unroll
    for( int q = 0; q < 2; q++ )
#pragma unroll
      for( int i = 0; i < 8; i++ )
      {
        int v = ( r + q < rEff && c0 + i < cEff ) ? acc[q][i] >> shift : 0;
        if( CLIP ) v = clip16( v );
        out[( r + q ) * oRowStride + ( c0 + i ) * oColStride] = v;
        if( sumAbs ) *sumAbs += abs( v );
      }
  }
}

// The same product for int16 A values with the summation index contiguous (rows of aRowStride samples, even): v_dot2c_i32_i16 takes two summation steps per
// instruction.  Bp: the matrix with rows n, n + 1 interleaved per column -- Bp[(n >> 1) * cols + c] = (B[n][c], B[n+1][c]).
template<int LPT, bool CLIP, class OutT>
__device__ __forceinline__ void tuq_pass16( const int16_t *A, int aRowStride, const unsigned *Bp, int inner, int rows, int cols, int rEff, int cEff, OutT *out,
                                            int oRowStride, int oColStride, int shift, int t )
{
  typedef short v2s __attribute__( ( ext_vector_type( 2 ) ) );
  const int cb = cols >> 3, lcb = 31 - __clz( cb ), rnd = shift > 0 ? 1 << ( shift - 1 ) : 0;
  for( int it = t; it < ( rows >> 1 ) * cb; it += LPT )
  {
    const int r = ( it >> lcb ) << 1, c0 = ( it & ( cb - 1 ) ) << 3;
    int       acc[2][8];
#pragma unroll
    for( int i = 0; i < 8; i++ ) acc[0][i] = acc[1][i] = rnd;
    if( r < rEff && c0 < cEff )
    {
      const unsigned *a0 = reinterpret_cast<const unsigned *>( A + r * aRowStride ), *a1 = reinterpret_cast<const unsigned *>( A + ( r + 1 ) * aRowStride );
      for( int n2 = 0; n2 < ( inner >> 1 ); n2++ )
      {
        const unsigned av0 = a0[n2], av1 = a1[n2];
        const uint4    b0 = *reinterpret_cast<const uint4 *>( Bp + n2 * cols + c0 ), b1 = *reinterpret_cast<const uint4 *>( Bp + n2 * cols + c0 + 4 );
        const unsigned bw[8] = { b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w };
        v2s va0, va1;
        __builtin_memcpy( &va0, &av0, 4 );
        __builtin_memcpy( &va1, &av1, 4 );
#pragma unroll
        for( int i = 0; i < 8; i++ )
        {
          v2s vb;
          __builtin_memcpy( &vb, &bw[i], 4 );
          acc[0][i] = __builtin_amdgcn_sdot2( va0, vb, acc[0][i], false );
          acc[1][i] = __builtin_amdgcn_sdot2( va1, vb, acc[1][i], false );
        }
      }
    }
#pragma unroll
    for( int q = 0; q < 2; q++ )
#pragma unroll
      for( int i = 0; i < 8; i++ )
      {
        int v = ( r + q < rEff && c0 + i < cEff ) ? acc[q][i] >> shift : 0;
        if( CLIP ) v = clip16( v );
        out[( r + q ) * oRowStride + ( c0 + i ) * oColStride] = ( OutT ) v;
      }
  }
}

// One N x N core matrix (N = 1 << lN, row-major M[k][n]) into the two slots a dimension of the blocked kernels has, by the whole workgroup (256 threads):
//   plain: M with rows k, k+1 interleaved        -- (M[k][n], M[k+1][n]) at pair-row k >> 1, column n: the inverse passes
//   trans: M^T with rows n, n+1 interleaved      -- (M[k][n], M[k][n+1]) at pair-row n >> 1, column k: the packed first forward pass, tuq_pass_il
//          or, TRANS_PLAIN, M^T as it is         -- the second forward pass of a non-square TU (32-bit input, tuq_pass)
template<bool TRANS_PLAIN>
__device__ __forceinline__ void tuq_stage_matrix( const int16_t *m, int N, int lN, int16_t *plain, int16_t *trans )
{
  for( int i = threadIdx.x; i < N * N; i += 256 )
  {
    const int k = i >> lN, n = i & ( N - 1 );
    plain[( ( k >> 1 ) * N + n ) * 2 + ( k & 1 )] = m[i];
    if( TRANS_PLAIN ) trans[n * N + k] = m[i];
    else trans[( ( n >> 1 ) * N + k ) * 2 + ( n & 1 )] = m[i];
  }
}

// ---- 4. generic LDS passes: lane t of `step` lanes, one output per trip, the matrix column / row contiguous in LDS -----------------------------------------------
constexpr int ALL_LINES = 0x7fffffff;   // linesEff of a pass that cuts no line (the comparison folds away)

// sMT[n * N + k] = M[k][n]
__device__ __forceinline__ void lds_load_matrix_T( const int16_t *m, int N, int16_t *sMT, int t, int step )
{
  for( int i = t; i < N * N; i += step )
  {
    const int k = i / N, n = i - k * N;
    sMT[n * N + k] = m[i];
  }
}

__device__ __forceinline__ void lds_load_matrix( const int16_t *m, int N, int16_t *sM, int t, int step )
{
  for( int i = t; i < N * N; i += step ) sM[i] = m[i];
}

// forward: dst[k * dstLd + j] = (sum_n M[k][n] * src[j * srcLd + n] + rnd) >> shift   for j < lines, k < N; zero for j >= linesEff or k >= kEff.
// sumAbs (may be null) collects |dst|.
template<class SumT>
__device__ __forceinline__ void lds_fwd_pass( const int *src, int srcLd, int *dst, int dstLd, const int16_t *sMT, int N, int lines, int linesEff, int kEff, int shift,
                                              int t, int step, SumT *sumAbs )
{
  const int rnd = shift > 0 ? 1 << ( shift - 1 ) : 0;
  for( int o = t; o < lines * N; o += step )
  {
    const int j = o / N, k = o - j * N;
    int       v = 0;
    if( j < linesEff && k < kEff )
    {
      unsigned sum = 0;
      for( int n = 0; n < N; n++ ) sum += ( unsigned ) src[j * srcLd + n] * ( unsigned ) ( int ) sMT[n * N + k];
      v = ( int ) ( sum + ( unsigned ) rnd ) >> shift;
    }
    dst[k * dstLd + j] = v;
    if( sumAbs ) *sumAbs += abs( v );
  }
}

// inverse: out( o, i, j, clip16( (sum_{k < cut} src[k * srcLd + i] * M[k][j] + rnd) >> shift ) )   for i < lines, j < N, o = i * N + j; zero for i >= linesEff.  sM[k * N + j] = M[k][j].
// out is the store of a first pass or the per-sample epilogue of the last one.
template<class Out>
__device__ __forceinline__ void lds_inv_pass( const int *src, int srcLd, const int16_t *sM, int N, int lines, int linesEff, int cut, int shift, int t, int step, Out out )
{
  const unsigned rnd = 1u << ( shift - 1 );
  for( int o = t; o < lines * N; o += step )
  {
    const int i = o / N, j = o - i * N;
    int       v = 0;
    if( i < linesEff )
    {
      unsigned sum = 0;
      for( int k = 0; k < cut; k++ ) sum += ( unsigned ) src[k * srcLd + i] * ( unsigned ) ( int ) sM[k * N + j];
      v = clip16( ( int ) ( sum + rnd ) >> shift );
    }
    out( o, i, j, v );
  }
}

// ---- 5. the 2-D transforms of the one-lane kernels: a W x H block (W * H <= 32, no zero-out at these sizes) in registers ---------------------------------------
// mh / mv: the W- / H-point core matrix of the job's horizontal / vertical type, row-major (LDS)
// forward: rows with the horizontal matrix, then columns with the vertical one; b[k * W + x] are the coefficients, sumAbs collects |b|
template<int W, int H>
__device__ __forceinline__ void lane_fwd_2d( const int ( &r )[W * H], int ( &b )[W * H], const int16_t *mh, const int16_t *mv, int bitDepth, long long &sumAbs )
{
  constexpr int LW = W == 4 ? 2 : 3, LH = H == 4 ? 2 : 3;
  const int     s1 = LW + bitDepth + 6 - 15, s2 = LH + 6;
  const int     rnd1 = s1 > 0 ? 1 << ( s1 - 1 ) : 0, rnd2 = 1 << ( s2 - 1 );
  int           t[W * H];
#pragma unroll
  for( int y = 0; y < H; y++ )
#pragma unroll
    for( int k = 0; k < W; k++ )
    {
      unsigned sum = 0;
#pragma unroll
      for( int n = 0; n < W; n++ ) sum += ( unsigned ) r[y * W + n] * ( unsigned ) ( int ) mh[k * W + n];
      t[k * H + y] = ( int ) ( sum + ( unsigned ) rnd1 ) >> s1;
    }
#pragma unroll
  for( int x = 0; x < W; x++ )
#pragma unroll
    for( int k = 0; k < H; k++ )
    {
      unsigned sum = 0;
#pragma unroll
      for( int n = 0; n < H; n++ ) sum += ( unsigned ) t[x * H + n] * ( unsigned ) ( int ) mv[k * H + n];
      const int v = ( int ) ( sum + ( unsigned ) rnd2 ) >> s2;
      b[k * W + x] = v;
      sumAbs += abs( v );
    }
}

// inverse: columns, then rows; out( y, x, v ) takes every reconstructed sample (row by row)
template<int W, int H, class Out>
__device__ __forceinline__ void lane_inv_2d( const int ( &b )[W * H], const int16_t *mh, const int16_t *mv, int bitDepth, Out out )
{
  const int      s2 = 20 - bitDepth;
  const unsigned rnd1 = 1u << 6, rnd2 = 1u << ( s2 - 1 );
  int            t[W * H];
#pragma unroll
  for( int x = 0; x < W; x++ )
#pragma unroll
    for( int y = 0; y < H; y++ )
    {
      unsigned sum = 0;
#pragma unroll
      for( int k = 0; k < H; k++ ) sum += ( unsigned ) b[k * W + x] * ( unsigned ) ( int ) mv[k * H + y];
      t[x * H + y] = clip16( ( int ) ( sum + rnd1 ) >> 7 );
    }
#pragma unroll
  for( int y = 0; y < H; y++ )
#pragma unroll
    for( int x = 0; x < W; x++ )
    {
      unsigned sum = 0;
#pragma unroll
      for( int k = 0; k < W; k++ ) sum += ( unsigned ) t[k * H + y] * ( unsigned ) ( int ) mh[k * W + x];
      out( y, x, clip16( ( int ) ( sum + rnd2 ) >> s2 ) );
    }
}

}   // namespace
