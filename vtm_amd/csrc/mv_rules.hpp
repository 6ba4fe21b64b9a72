// mv_rules.hpp -- the reference's motion-vector rules as device functions, one definition each (reference CommonLib/Mv.*, CommonLib/RdCost.h,
// EncoderLib/InterSearch.cpp).  Every search kernel must agree with the reference bit for bit, so every kernel takes them from here.
#pragma once
#include <hip/hip_runtime.h>

namespace mvr
{

// floorLog2 of v >= 1
__device__ __forceinline__ int floor_log2_u( unsigned v ) { return 31 - __clz( ( int ) v ); }

// xGetExpGolombNumberOfBits (RdCost.h:301-313): its `while( t > 128 ) { len += 14; t >>= 7; }` only splits floorLog2( t ) = 7 + floorLog2( t >> 7 ),
// so the length is 1 + 2 * floorLog2( t ) for every t >= 1 -- no loop
__device__ __forceinline__ unsigned eg_bits( int v )
{
  const unsigned t = ( v <= 0 ) ? ( ( unsigned ) ( -v ) << 1 ) + 1 : ( unsigned ) ( v << 1 );
  return 1u + ( ( unsigned ) ( 31 - __clz( ( int ) t ) ) << 1 );
}
// getBitsOfVectorWithPredictor (RdCost.h:314-315) with m_iCostScale = costScale
__device__ __forceinline__ unsigned mv_bits( int x, int y, int predHor, int predVer, int costScale, unsigned imvShift )
{
  return eg_bits( ( ( x << costScale ) - predHor ) >> imvShift ) + eg_bits( ( ( y << costScale ) - predVer ) >> imvShift );
}
// RdCost::getCost: fp64 multiply, truncation
__device__ __forceinline__ unsigned long long rate( double lambda, unsigned bits ) { return ( unsigned long long ) ( lambda * bits ); }

// Mv::changePrecision to a coarser precision (Mv.h:183-197), rs >= 1
__device__ __forceinline__ int prec_down( int v, int rs ) { const int o = 1 << ( rs - 1 ); return v >= 0 ? ( v + o - 1 ) >> rs : ( v + o ) >> rs; }
// the same where rs may be 0 (the affine AMVR mode of 1/16 precision): v unchanged
__device__ __forceinline__ int prec_down_or_keep( int v, int rs ) { if( rs == 0 ) return v; return prec_down( v, rs ); }

// cu.imv -> the shift from MV_PRECISION_INTERNAL (1/16) to the AMVR precision (Mv::m_amvrPrecision): quarter, integer, 4-sample, half
__device__ __forceinline__ int amvr_shift( int imv ) { return imv == 0 ? 2 : imv == 1 ? 4 : imv == 2 ? 6 : 3; }
// imvShift of the quarter-sample searches (RdCost::setCostScale / getBitsOfVectorWithPredictor): the AMVR shift less MV_FRACTIONAL_BITS_DIFF
__device__ __forceinline__ unsigned imv_shift( int imv ) { return imv == 3 ? 1u : ( unsigned ) imv << 1; }
// the AMVR shift of an affine block (rsTab of InterSearch::xAffineMotionEstimation): quarter, 1/16, integer
__device__ __forceinline__ int affine_amvr_shift( int imv ) { return imv == 0 ? 2 : imv == 1 ? 0 : 4; }

// clipMvInPic (Mv.cpp:56-74): the limits of a vector component (1/16 precision) of a PU at luma position pos; size: the picture's width (height).
// Macros, not functions: written into the caller's expression, the bound arithmetic folds with the caller's 16-bit position fields exactly as before; through
// an int parameter the compiler canonicalises it differently and the TZ / full-search / xMotionEstimation kernels change.
#define MVR_CLIP_MAX( size, pos ) ( ( ( size ) + 8 - ( pos ) - 1 ) << 4 )
#define MVR_CLIP_MIN( ctuSize, pos ) ( ( -( ctuSize ) - 8 - ( pos ) + 1 ) << 4 )
__device__ __forceinline__ int mv_clip_axis( int v, int size, int ctuSize, int pos ) { return min( MVR_CLIP_MAX( size, pos ), max( MVR_CLIP_MIN( ctuSize, pos ), v ) ); }

// removeWeightHighFreq (Buffer.h:417-460) under BCW weight bcw (of g_BcwWeightBase = 8; not the default pair, not 0): ( org * w0 - pred * w1 + 2^15 ) >> 16
__device__ __forceinline__ int bcw_normaliser( int bcw ) { return ( ( 1 << 16 ) + ( bcw > 0 ? ( bcw >> 1 ) : -( bcw >> 1 ) ) ) / bcw; }
__device__ __forceinline__ int bcw_w0( int nrm ) { return nrm << 3; }
__device__ __forceinline__ int bcw_w1( int bcw, int nrm ) { return ( 8 - bcw ) * nrm; }

// xGetMEDistortionWeight (InterSearch.cpp:7666-7676): |getBcwWeight| / g_BcwWeightBase of a bi search, 0.5 for the default pair; bcwDefault: the value the
// caller uses for that pair
__device__ __forceinline__ double me_dist_weight( bool bi, int bcw, int bcwDefault ) { return bi ? ( bcw != bcwDefault ? fabs( ( double ) bcw / 8.0 ) : 0.5 ) : 1.0; }

// xEstimateMvPredAMVP's selection (InterSearch.cpp:3088-3128): the cost of AMVP candidate c is its template SAD plus the rate of its index bits, and the FIRST candidate
// with the smallest cost wins
__device__ __forceinline__ unsigned long long amvp_cost( unsigned long long sad, double lambda, unsigned idxBits ) { return sad + rate( lambda, idxBits ); }
// the pick between two costs (c1 = ~0: no second candidate)
__device__ __forceinline__ int amvp_pick( unsigned long long c0, unsigned long long c1 ) { return c0 > c1 ? 1 : 0; }

}   // namespace mvr
