// lmcs.hpp -- the two sample rules of LMCS chroma residual scaling, AreaBuf<Pel>::scaleSignal (reference CommonLib/Buffer.cpp:415-464), defined once for
// every kernel that applies them (lmcs.hip, the CRS instantiations of the chains in transform.hip and jccr.hip).  CSCALE_FP_PREC = 11, M = (1 << bitDepth) - 1:
//   forward (dir 1):  a = |v|;  out = Pel( Clip3( -M, M, sgn(v) * ( ((a << 11) + (scale >> 1)) / scale ) ) )        `/` truncates; sgn(0) = +1
//   inverse (dir 0):  c = Clip3( -M-1, M, v );  a = |c|;  out = Clip3( -32768, 32767, sgn(c) * ( (a * scale + 1024) >> 11 ) )
// Scale contract: 1 <= scale <= 32767 (ChromaScaleCoeff lies in 256 .. 16384, 2048 for empty bins); v: any int16; bitDepth <= 12.
#pragma once
#include <cstdint>

#define LMCS_CSCALE_FP_PREC 11

// The forward rule divides by the job's scale.  The quotient comes from one reciprocal per job and one correction per sample:
//   magic = floor( (2^32 - 1) / scale ),  2^32 - 1 = magic * scale + r,  0 <= r < scale
//   q0    = floor( N * magic / 2^32 ) = floor( N / scale - e ),  e = N * (1 + r) / (scale * 2^32) <= N / 2^32
// N = (a << 11) + (scale >> 1) < 2^26 + 2^11 + 2^14 < 2^27 for every int16 sample (a <= 32768), so 0 <= e < 2^-5 < 1 and q0 is floor( N / scale ) or one
// below it.  N - q0 * scale then lies in [0, 2 * scale) (no 32-bit wrap: it is below 2^16) and is >= scale exactly when q0 is one short: one conditional
// increment makes the quotient exact for every N < 2^32 / 2^5 and every scale of the contract, scale = 1 included (magic = 2^32 - 1, r = 0).
struct LmcsScale
{
  unsigned scale, magic;
};

__host__ __device__ __forceinline__ LmcsScale lmcs_scale_of( int scale )
{
  LmcsScale s;
  s.scale = ( unsigned ) scale;
  s.magic = 0xffffffffu / ( unsigned ) scale;
  return s;
}

__device__ __forceinline__ int lmcs_fwd( int v, const LmcsScale &s, int maxAbs )
{
  const unsigned a = ( unsigned ) ( v < 0 ? -v : v );
  const unsigned n = ( a << LMCS_CSCALE_FP_PREC ) + ( s.scale >> 1 );
  unsigned       q = __umulhi( n, s.magic );
  q += n - q * s.scale >= s.scale ? 1u : 0u;
  const int r = ( int ) ( q < ( unsigned ) maxAbs ? q : ( unsigned ) maxAbs );   // Clip3( -M, M, sgn * q ) = sgn * min( q, M )
  return v < 0 ? -r : r;
}

__device__ __forceinline__ int lmcs_inv( int v, int scale, int maxAbs )
{
  const int c = v < -maxAbs - 1 ? -maxAbs - 1 : v > maxAbs ? maxAbs : v;
  const int a = c < 0 ? -c : c;                                                        // <= 4096: a * scale + 1024 < 2^27
  const int r = ( a * scale + ( 1 << ( LMCS_CSCALE_FP_PREC - 1 ) ) ) >> LMCS_CSCALE_FP_PREC;
  const int o = c < 0 ? -r : r;
  return o < -32768 ? -32768 : o > 32767 ? 32767 : o;
}

// A chain job's chroma adjustment as the CRS instantiations use it: 0 = leave the samples alone.  The reference scales a chroma TU only when
// width * height > 4 (InterSearch.cpp:6628, 6728, 6838, 6978); a value outside 1 .. 32767 counts as 0.
__device__ __forceinline__ int lmcs_job_adj( int adj, int width, int height ) { return ( adj >= 1 && adj <= 32767 && width * height > 4 ) ? adj : 0; }
