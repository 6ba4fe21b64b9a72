// geo_host.hpp -- the GEO merge estimation of one CU as host arithmetic, without a HIP dependency: the bodies of vtmhip_geo_host and vtmhip_geo_tables_host
// (geo.hip), which host/test_geo_cand.cpp compiles with g++ under the sanitizers.  The rules are geo_rules.hpp's; the two costs of a block are ciipHostCosts
// (ciip_host.hpp: the Hadamard tile by had_tile_rule.hpp, evaluated as had_finish evaluates it on the device).
#pragma once
#include <algorithm>
#include <vector>

#include "geo_rules.hpp"
#include "ciip_host.hpp"

namespace
{

constexpr uint64_t GEO_HOST_NO_COST = ~( uint64_t ) 0;

inline int geoHostTables( int splitDir, int w, int h, int chroma, int16_t *weightOut, int16_t *maskOut )
{
  if( !geoSizeOk( w, h ) || splitDir < 0 || splitDir >= GEO_NUM_SPLIT || chroma < 0 || chroma > 1 ) return -1;
  if( weightOut )
  {
    const GeoLine l = geoLine( splitDir, w, h, chroma, chroma );
    const int     bw = w >> chroma, bh = h >> chroma;
    for( int y = 0; y < bh; y++ )
      for( int x = 0; x < bw; x++ ) weightOut[y * bw + x] = ( int16_t ) geoWeightOfIdx( geoLineIdx( l, x, y ) );
  }
  if( maskOut )
  {
    const GeoLine l = geoLine( splitDir, w, h, 0, 0 );
    for( int y = 0; y < h; y++ )
      for( int x = 0; x < w; x++ ) maskOut[y * w + x] = ( int16_t ) geoMaskOfIdx( geoLineIdx( l, x, y ) );
  }
  return 0;
}

struct GeoHostKey { uint64_t bits; int order; };

// 0, or -1 for a job the table predicate rejects or a missing pointer: nothing is written then
inline int geoHostJob( const vtmhip_geo_job *job, const int16_t *orgBase, const int16_t *const pred[VTMHIP_GEO_MAX_CAND], int useSatd, vtmhip_geo_result *res,
                       uint64_t *sadSplit, int16_t *blend )
{
  if( !job || !orgBase || !pred || !res ) return -1;
  if( !geoJobOk( *job, 64, 64, true ) ) return -1;
  for( int k = 0; k < job->numCand; k++ )
    if( !pred[k] ) return -1;
  const int      w = job->width, h = job->height, bd = job->bitDepth, n = job->numCand, os = job->orgStride, pairs = geoNumPairs( n );
  const int16_t *org = orgBase + job->orgOff;
  const double   lambda = job->sqrtLambda;

  memset( res, 0, sizeof( *res ) );
  std::vector<uint16_t> diff( ( size_t ) VTMHIP_GEO_MAX_CAND * w * h );   // | org - rounded candidate |, formed once
  std::vector<uint64_t> sadLarge( ( size_t ) GEO_NUM_SPLIT * VTMHIP_GEO_MAX_CAND, GEO_HOST_NO_COST );
  for( int c = 0; c < VTMHIP_GEO_MAX_CAND; c++ )
  {
    res->sadWhole[c] = GEO_HOST_NO_COST;
    if( c >= n ) continue;
    uint64_t s = 0;
    for( int y = 0; y < h; y++ )
      for( int x = 0; x < w; x++ )
      {
        const int d = abs( ( int ) org[y * os + x] - geoRoundSample( pred[c][y * w + x], bd ) );
        diff[( size_t ) c * w * h + y * w + x] = ( uint16_t ) d;
        s += ( uint64_t ) d;
      }
    res->sadWhole[c] = s;
  }
  for( int split = 0; split < GEO_NUM_SPLIT; split++ )
  {
    const GeoLine l = geoLine( split, w, h, 0, 0 );
    for( int c = 0; c < n; c++ )
    {
      uint64_t s = 0;
      for( int y = 0; y < h; y++ )
        for( int x = 0; x < w; x++ )
          if( geoMaskOfIdx( geoLineIdx( l, x, y ) ) ) s += diff[( size_t ) c * w * h + y * w + x];
      sadLarge[split * VTMHIP_GEO_MAX_CAND + c] = s;
    }
  }
  if( sadSplit ) memcpy( sadSplit, sadLarge.data(), sizeof( uint64_t ) * sadLarge.size() );

  const double            best = geoBestWholeCost( res->sadWhole, n, lambda );
  std::vector<GeoHostKey> list;
  for( int split = 0; split < GEO_NUM_SPLIT; split++ )
    for( int p = 0; p < pairs; p++ )
    {
      int c0, c1;
      geoPair( p, c0, c1 );
      const uint64_t l0 = sadLarge[split * VTMHIP_GEO_MAX_CAND + c0], l1 = sadLarge[split * VTMHIP_GEO_MAX_CAND + c1];
      double         cost;
      if( geoComboCost( geoSideCost( l0, c0, lambda ), geoSideCost( res->sadWhole[c1] - l1, c1, lambda ), best, lambda, cost ) )
        list.push_back( GeoHostKey{ geoCostBits( cost ), geoOrderOf( split, p ) } );
    }
  std::sort( list.begin(), list.end(), []( const GeoHostKey &a, const GeoHostKey &b ) { return geoComboBefore( a.bits, a.order, b.bits, b.order ); } );
  res->numPassed = ( int32_t ) list.size();
  res->numTested = ( int32_t ) std::min<size_t>( list.size(), VTMHIP_GEO_MAX_TRY );

  std::vector<int16_t> cur( ( size_t ) w * h );
  for( int r = 0; r < VTMHIP_GEO_MAX_TRY; r++ )
  {
    vtmhip_geo_combo &o = res->combo[r];
    o.dist = GEO_HOST_NO_COST;
    if( r >= res->numTested ) continue;
    const int split = list[r].order >> 5;
    int       c0, c1;
    geoPair( list[r].order & 31, c0, c1 );
    o.splitDir = ( uint8_t ) split; o.cand0 = ( uint8_t ) c0; o.cand1 = ( uint8_t ) c1;
    memcpy( &o.cost, &list[r].bits, sizeof( double ) );
    const GeoLine l = geoLine( split, w, h, 0, 0 );
    for( int y = 0; y < h; y++ )
      for( int x = 0; x < w; x++ ) cur[y * w + x] = ( int16_t ) geoBlendSample( geoWeightOfIdx( geoLineIdx( l, x, y ) ), pred[c0][y * w + x], pred[c1][y * w + x], bd );
    uint64_t satd, sad;
    ciipHostCosts( org, os, cur.data(), w, h, satd, sad );
    o.dist = useSatd ? satd : sad;
    if( blend ) memcpy( blend + ( size_t ) r * w * h, cur.data(), sizeof( int16_t ) * w * h );
  }
  return 0;
}

}   // namespace
