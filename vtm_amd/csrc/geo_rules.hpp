// geo_rules.hpp -- the rules of the geometric partitioning mode (GEO) of the reference's merge estimation, defined once for host and device: plain functions without
// a HIP dependency, so host/test_geo_cand.cpp compiles them with g++ and the kernels of geo.hip use the same text.
//   geoDis / geoAngle2Mask / geoAngle2Mirror   the three 32-entry tables of the standard                                  CommonLib/Rom.cpp:786-788
//   geoSplitParams        the 64 (angle, distance) pairs of initGeoTemplate                                                 Rom.cpp:703-718
//   geoWeightOffset       g_weightOffset as arithmetic                                                                      Rom.cpp:749-776
//   geoSizeOk             the eligible sizes: sides 8 .. 64, w < 8h, h < 8w (14 shapes)                                      EncModeCtrl.cpp:1646-1648
//   geoLine               the weight index of a block's samples as c0 + cx * x + cy * y: the closed form of a plane entry (Rom.cpp:730-745) at the address the three
//                         mirror cases of xWeightedGeoBlk (InterpolationFilter.cpp:923-956) and of the masked SAD's set-up (EncCu.cpp:2924-2948) walk to.  The two
//                         walks differ in their stride signs (the SAD adds maskStride and maskStride2 per row, the blend one stepY) and arrive at the same plane
//                         entry for a luma sample; the 4:2:0 chroma walk steps the plane by two
//   geoWeight / geoSadMask   Clip3( 0, 8, ( 32 + wIdx + 4 ) >> 3 ) and wIdx > 0
//   geoBlendSample        the sample rule of xWeightedGeoBlk                                                                InterpolationFilter.cpp:915-919, :949
//   geoRoundSample        PelBuf::roundToOutputBitdepth, one sample                                                         Buffer.cpp:585-613
//   geoPair               the pair order m_GeoModeTest                                                                      EncCu.cpp:62-70
//   geoSideCost / geoBestWholeCost / geoComboCost   the first-pass costs in double, exactly as written (EncCu.cpp:2905-2910, :2956-2958, :2972-2976): every
//                         translation unit that includes this file is compiled without contraction (-ffp-contract=off)
//   geoComboBefore        the list order: ascending cost, ties by splitDir, then by index in the pair order -- a total order, one valid outcome of the reference's
//                         unstable std::sort (EncCu.h:87-100), and the project's rule
//   geoJobOk / geoBlendJobOk   what a row of the two device tables must satisfy before anything is read through it
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/vtmhip.h"

#if defined( __HIPCC__ )
#define GEO_HD __host__ __device__ inline
#else
#define GEO_HD inline
#endif

enum { GEO_NUM_SPLIT = 64, GEO_PLANE = 112, GEO_PLANE_OFFSET = 8, GEO_MAX_PAIRS = 30, GEO_MAX_COMBOS = GEO_NUM_SPLIT * GEO_MAX_PAIRS, GEO_BITS_SPLIT = 6 };

GEO_HD int geoDis( int a )
{
  const int8_t t[32] = { 8, 8, 8, 8, 4, 4, 2, 1, 0, -1, -2, -4, -4, -8, -8, -8, -8, -8, -8, -8, -4, -4, -2, -1, 0, 1, 2, 4, 4, 8, 8, 8 };
  return t[a & 31];
}
GEO_HD int geoAngle2Mask( int a )
{
  const int8_t t[32] = { 0, -1, 1, 2, 3, 4, -1, -1, 5, -1, -1, 4, 3, 2, 1, -1, 0, -1, 1, 2, 3, 4, -1, -1, 5, -1, -1, 4, 3, 2, 1, -1 };
  return t[a & 31];
}
GEO_HD int geoAngle2Mirror( int a )
{
  const int8_t t[32] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 2, 2, 2, 2 };
  return t[a & 31];
}

// the splitDir-th pair that initGeoTemplate keeps; false beyond the 64th
GEO_HD bool geoSplitParams( int splitDir, int &angle, int &distance )
{
  int mode = 0;
  for( int a = 0; a < 32; a++ )
    for( int d = 0; d < 4; d++ )
    {
      const int m = geoAngle2Mask( a );
      if( ( d == 0 && a >= 16 ) || ( ( d == 2 || d == 0 ) && ( m == 0 || m == 5 ) ) || m == -1 ) continue;
      if( mode++ == splitDir ) { angle = a; distance = d; return true; }
    }
  return false;
}

GEO_HD bool geoSideOk( int s ) { return s == 8 || s == 16 || s == 32 || s == 64; }
GEO_HD bool geoSizeOk( int w, int h ) { return geoSideOk( w ) && geoSideOk( h ) && w < 8 * h && h < 8 * w; }

GEO_HD void geoWeightOffset( int angle, int distance, int w, int h, int &ox, int &oy )
{
  ox = ( GEO_PLANE - w ) >> 1;
  oy = ( GEO_PLANE - h ) >> 1;
  if( distance > 0 )
  {
    if( angle % 16 == 8 || ( angle % 16 != 0 && h >= w ) ) oy += angle < 16 ? ( distance * h ) >> 3 : -( ( distance * h ) >> 3 );
    else ox += angle < 16 ? ( distance * w ) >> 3 : -( ( distance * w ) >> 3 );
  }
}

// the angle whose plane initGeoTemplate stores for this angle's mask: the first of 0 .. 8 with the same g_angle2mask entry
GEO_HD int geoPlaneAngle( int angle )
{
  const int m = geoAngle2Mask( angle );
  for( int a = 0; a <= 8; a++ )
    if( geoAngle2Mask( a ) == m ) return a;
  return 0;
}

// the plane entry at ( px, py ) of the plane of `planeAngle` before the clip: weightIdx of Rom.cpp:741
GEO_HD int geoPlaneIdx( int planeAngle, int px, int py )
{
  const int dx = geoDis( planeAngle ), dy = geoDis( ( planeAngle + 8 ) % 32 );
  return ( 2 * ( px + GEO_PLANE_OFFSET ) + 1 ) * dx + ( 2 * ( py + GEO_PLANE_OFFSET ) + 1 ) * dy - ( dx + dy ) * 128;   // rho: ( dis << 7 ) for both, as a product (dis may be negative)
}

struct GeoLine { int c0, cx, cy; };   // weightIdx of the block's sample ( x, y ) = c0 + cx * x + cy * y

// cuW x cuH: the CU's LUMA size; scaleX / scaleY: 0 for luma, 1 for a 4:2:0 chroma block, whose sample ( x, y ) reads the plane two entries apart
GEO_HD GeoLine geoLine( int splitDir, int cuW, int cuH, int scaleX, int scaleY )
{
  int angle = 0, distance = 0, ox, oy;
  geoSplitParams( splitDir, angle, distance );
  geoWeightOffset( angle, distance, cuW, cuH, ox, oy );
  const int mirror = geoAngle2Mirror( angle ), pa = geoPlaneAngle( angle );
  const int px0 = mirror == 1 ? GEO_PLANE - 1 - ox : ox, py0 = mirror == 2 ? GEO_PLANE - 1 - oy : oy;
  const int sx = mirror == 1 ? -( 1 << scaleX ) : 1 << scaleX, sy = mirror == 2 ? -( 1 << scaleY ) : 1 << scaleY;
  GeoLine   l;
  l.c0 = geoPlaneIdx( pa, px0, py0 );
  l.cx = geoPlaneIdx( pa, px0 + sx, py0 ) - l.c0;
  l.cy = geoPlaneIdx( pa, px0, py0 + sy ) - l.c0;
  return l;
}
GEO_HD int geoLineIdx( const GeoLine &l, int x, int y ) { return l.c0 + l.cx * x + l.cy * y; }
GEO_HD int geoWeightOfIdx( int wIdx )
{
  const int v = ( 32 + wIdx + 4 ) >> 3;
  return v < 0 ? 0 : v > 8 ? 8 : v;
}
GEO_HD int geoMaskOfIdx( int wIdx ) { return wIdx > 0; }

// the rule of one sample, stated whole: each call walks the split list and forms the line again.  Loops over a block -- every device loop, the host entries --
// form the GeoLine once and evaluate geoLineIdx per sample
GEO_HD int geoWeight( int splitDir, int cuW, int cuH, int x, int y, int scaleX, int scaleY ) { return geoWeightOfIdx( geoLineIdx( geoLine( splitDir, cuW, cuH, scaleX, scaleY ), x, y ) ); }
GEO_HD int geoSadMask( int splitDir, int cuW, int cuH, int x, int y ) { return geoMaskOfIdx( geoLineIdx( geoLine( splitDir, cuW, cuH, 0, 0 ), x, y ) ); }

GEO_HD int geoBlendSample( int weight, int s0, int s1, int bitDepth )
{
  const int shift = ( 14 - bitDepth > 2 ? 14 - bitDepth : 2 ) + 3, offset = ( 1 << ( shift - 1 ) ) + ( 8192 << 3 ), maxVal = ( 1 << bitDepth ) - 1;
  const int v = ( weight * s0 + ( 8 - weight ) * s1 + offset ) >> shift;
  return v < 0 ? 0 : v > maxVal ? maxVal : v;
}
GEO_HD int geoRoundSample( int s, int bitDepth )
{
  const int shift = 14 - bitDepth > 2 ? 14 - bitDepth : 2, maxVal = ( 1 << bitDepth ) - 1;
  const int v = ( s + ( 1 << ( shift - 1 ) ) + 8192 ) >> shift;
  return v < 0 ? 0 : v > maxVal ? maxVal : v;
}

// m_GeoModeTest: for k = 1 .. 5 the pairs ( 0 .. k - 1, k ), then ( k, 0 .. k - 1 ); a CU with numCand candidates tests the first numCand * ( numCand - 1 )
GEO_HD void geoPair( int idx, int &cand0, int &cand1 )
{
  int k = 1;
  while( ( k + 1 ) * k <= idx ) k++;
  const int i = idx - k * ( k - 1 );
  if( i < k ) { cand0 = i; cand1 = k; }
  else { cand0 = k; cand1 = i - k; }
}
GEO_HD int geoNumPairs( int numCand ) { return numCand * ( numCand - 1 ); }

GEO_HD double geoSideCost( uint64_t sad, int cand, double sqrtLambda ) { return ( double ) sad + ( double ) ( cand + 1 ) * sqrtLambda; }
// the cost of the first strict minimum of the whole-block SADs
GEO_HD double geoBestWholeCost( const uint64_t *sadWhole, int numCand, double sqrtLambda )
{
  uint64_t best = ~( uint64_t ) 0;
  double   cost = 1.7e308;
  for( int c = 0; c < numCand; c++ )
    if( sadWhole[c] < best ) { best = sadWhole[c]; cost = geoSideCost( best, c, sqrtLambda ); }
  return cost;
}
// false: the combination is dropped; true: cost is its list cost
GEO_HD bool geoComboCost( double cost0, double cost1, double bestWholeBlkCost, double sqrtLambda, double &cost )
{
  double t = cost0 + cost1;
  if( t > bestWholeBlkCost ) return false;
  t    = t + ( double ) GEO_BITS_SPLIT * sqrtLambda;
  cost = t;
  return true;
}

// the costs of a list are finite and not negative: their order is the order of their bit patterns.  order = splitDir * 32 + index in the pair order
GEO_HD uint64_t geoCostBits( double c )
{
  uint64_t u;
  memcpy( &u, &c, sizeof( u ) );
  return u;
}
GEO_HD int  geoOrderOf( int splitDir, int pairIdx ) { return splitDir * 32 + pairIdx; }
GEO_HD bool geoComboBefore( uint64_t costBitsA, int orderA, uint64_t costBitsB, int orderB ) { return costBitsA < costBitsB || ( costBitsA == costBitsB && orderA < orderB ); }

GEO_HD bool geoLambdaOk( double l ) { return l >= 0.0 && l <= 1.7e308; }   // finite and not negative (a NaN fails both)

// hasPred: the call has a d_predBase
GEO_HD bool geoJobOk( const vtmhip_geo_job &j, int maxW, int maxH, bool hasPred )
{
  if( !geoSizeOk( j.width, j.height ) || j.width > maxW || j.height > maxH || j.bitDepth < 8 || j.bitDepth > 12 ) return false;
  if( j.numCand < 2 || j.numCand > VTMHIP_GEO_MAX_CAND || j.orgStride < j.width || !geoLambdaOk( j.sqrtLambda ) ) return false;
  for( int k = 0; k < j.numCand; k++ )
    if( j.cand[k].refStride < j.width || ( j.cand[k].keepOff >= 0 && !hasPred ) ) return false;
  return true;
}

GEO_HD bool geoBlendJobOk( const vtmhip_geo_cu_blend_job &j )
{
  if( !geoSizeOk( j.width, j.height ) || j.bitDepth < 8 || j.bitDepth > 12 || j.splitDir >= GEO_NUM_SPLIT || j.chroma > 1 ) return false;
  const int bw = j.width >> j.chroma;
  return j.src0Stride >= bw && j.src1Stride >= bw && j.dstStride >= bw;
}
