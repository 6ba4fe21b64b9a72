// test_geo_cand.cpp -- the GEO rules of vtm_amd/csrc/geo_rules.hpp and the host entries' bodies of geo_host.hpp (both HIP-free) as a stand-alone program under
// AddressSanitizer and UBSan, compiled without contraction as the device code is (tests/test_geo_cand_cpp.py builds and runs it).  Every eligible shape, 8 .. 12 bit,
// 2 .. 6 candidates, lambdas for an empty, a short and a capped list: the original, the 14-bit blocks and the outputs sit in heap arrays of exactly their length,
// so a read or write past one is a report.  What the entries leave is checked for what can be said without a second implementation: the tables' ranges and their
// agreement with the plane form written out from its definition, the split and pair lists as permutations of what they enumerate, sadLarge between 0 and the whole
// SAD, the list strictly ascending under the stated order, every listed cost recomputed from the SADs, the blend between its inputs, the cap and the unused slots;
// then the predicate's edge jobs: each malformed field rejected with nothing written, each edge value accepted.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <random>

#include "../vtm_amd/csrc/geo_host.hpp"

static int g_failures = 0;
#define EXPECT( cond ) do { if( !( cond ) ) { g_failures++; if( g_failures < 20 ) printf( "FAIL %s:%d %s\n", __FILE__, __LINE__, #cond ); } } while( 0 )

template<class T> static std::unique_ptr<T[]> heap( size_t n ) { return std::unique_ptr<T[]>( new T[n]() ); }

static const int SIDES[4] = { 8, 16, 32, 64 };

static vtmhip_geo_job make_job( int w, int h, int bd, int numCand, double lambda )
{
  vtmhip_geo_job j = vtmhip_geo_job();
  j.width = ( int16_t ) w; j.height = ( int16_t ) h; j.bitDepth = ( uint8_t ) bd; j.numCand = ( uint8_t ) numCand; j.orgStride = w; j.sqrtLambda = lambda;
  for( int k = 0; k < VTMHIP_GEO_MAX_CAND; k++ ) { j.cand[k].refStride = w; j.cand[k].keepOff = -1; }
  return j;
}

static int pair_index( int c0, int c1 )
{
  for( int p = 0; p < GEO_MAX_PAIRS; p++ )
  {
    int a, b;
    geoPair( p, a, b );
    if( a == c0 && b == c1 ) return p;
  }
  return -1;
}

static void check_tables()
{
  // the split list: 64 distinct pairs, each with a mask; the pair list: every ordered pair of distinct candidates once, the first n ( n - 1 ) below n
  bool seenSplit[32][4] = {};
  int  a, d;
  for( int s = 0; s < GEO_NUM_SPLIT; s++ )
  {
    EXPECT( geoSplitParams( s, a, d ) && a >= 0 && a < 32 && d >= 0 && d < 4 && geoAngle2Mask( a ) >= 0 && !seenSplit[a][d] );
    seenSplit[a][d] = true;
  }
  EXPECT( !geoSplitParams( GEO_NUM_SPLIT, a, d ) );
  bool seenPair[6][6] = {};
  for( int p = 0; p < GEO_MAX_PAIRS; p++ )
  {
    int c0, c1;
    geoPair( p, c0, c1 );
    EXPECT( c0 >= 0 && c0 < 6 && c1 >= 0 && c1 < 6 && c0 != c1 && !seenPair[c0][c1] );
    seenPair[c0][c1] = true;
    for( int n = 2; n <= 6; n++ ) EXPECT( ( p < geoNumPairs( n ) ) == ( c0 < n && c1 < n ) );
  }
  int shapes = 0;
  for( int wi = 0; wi < 4; wi++ )
    for( int hi = 0; hi < 4; hi++ )
    {
      const int w = SIDES[wi], h = SIDES[hi];
      if( !geoSizeOk( w, h ) ) continue;
      shapes++;
      for( int s = 0; s < GEO_NUM_SPLIT; s++ )
        for( int chroma = 0; chroma < 2; chroma++ )
        {
          const int bw = w >> chroma, bh = h >> chroma;
          auto      wt = heap<int16_t>( ( size_t ) bw * bh ), mk = heap<int16_t>( ( size_t ) w * h );
          EXPECT( geoHostTables( s, w, h, chroma, wt.get(), mk.get() ) == 0 );
          int ox, oy, ones = 0;
          geoSplitParams( s, a, d );
          geoWeightOffset( a, d, w, h, ox, oy );
          EXPECT( ox >= 0 && ox + w <= GEO_PLANE && oy >= 0 && oy + h <= GEO_PLANE );   // the block lies inside the plane
          for( int y = 0; y < bh; y++ )
            for( int x = 0; x < bw; x++ )
            {
              EXPECT( wt[y * bw + x] >= 0 && wt[y * bw + x] <= 8 );
              EXPECT( wt[y * bw + x] == geoWeight( s, w, h, x, y, chroma, chroma ) );
              if( !chroma ) EXPECT( mk[y * w + x] == ( geoLineIdx( geoLine( s, w, h, 0, 0 ), x, y ) > 0 ) && ( mk[y * w + x] == 0 || wt[y * w + x] >= 4 ) );
            }
          for( int i = 0; i < w * h; i++ ) ones += mk[i];
          EXPECT( ones > 0 && ones < w * h );   // a split leaves both parts non-empty
        }
    }
  EXPECT( shapes == 14 );
  EXPECT( geoHostTables( 64, 8, 8, 0, nullptr, nullptr ) != 0 && geoHostTables( 0, 64, 8, 0, nullptr, nullptr ) != 0 && geoHostTables( 0, 8, 8, 2, nullptr, nullptr ) != 0 );
}

static long check_jobs( std::mt19937 &rng )
{
  long jobs = 0;
  int  regimes[3] = { 0, 0, 0 };
  for( int wi = 0; wi < 4; wi++ )
    for( int hi = 0; hi < 4; hi++ )
    {
      const int w = SIDES[wi], h = SIDES[hi];
      if( !geoSizeOk( w, h ) ) continue;
      for( int bd = 8; bd <= 12; bd++ )
        for( int numCand = 2; numCand <= 6; numCand++ )
        {
          const int    maxVal = ( 1 << bd ) - 1, shift = 14 - bd > 2 ? 14 - bd : 2, kind = ( int ) ( jobs % 3 );
          const double lambda = kind == 0 ? 0.0 : kind == 1 ? 4.0 + ( rng() % 1000 ) / 16.0 : 1.0e6;
          auto         org = heap<int16_t>( ( size_t ) w * h ), blend = heap<int16_t>( ( size_t ) VTMHIP_GEO_MAX_TRY * w * h );
          auto         split = heap<uint64_t>( ( size_t ) GEO_NUM_SPLIT * VTMHIP_GEO_MAX_CAND );
          auto         res = heap<vtmhip_geo_result>( 1 );
          std::unique_ptr<int16_t[]> pred[VTMHIP_GEO_MAX_CAND];
          const int16_t             *predPtr[VTMHIP_GEO_MAX_CAND] = {};
          for( int i = 0; i < w * h; i++ ) org[i] = ( int16_t ) ( rng() % ( maxVal + 1 ) );
          for( int k = 0; k < numCand; k++ )
          {
            pred[k] = heap<int16_t>( ( size_t ) w * h );
            // a 14-bit intermediate: ( sample << shift ) - 8192; near the original on one side of the block so that splits differ
            for( int i = 0; i < w * h; i++ )
            {
              const int near = ( ( i % w ) * ( k + 1 ) + ( i / w ) * ( 6 - k ) ) % ( w + h ) < ( w + h ) / 2;
              int       v = near ? org[i] + ( int ) ( rng() % 5 ) - 2 : ( int ) ( rng() % ( maxVal + 1 ) );
              v = v < 0 ? 0 : v > maxVal ? maxVal : v;
              pred[k][i] = ( int16_t ) ( ( v << shift ) - 8192 + ( int ) ( rng() % ( 1 << shift ) ) - ( 1 << ( shift - 1 ) ) );
            }
            predPtr[k] = pred[k].get();
          }
          const vtmhip_geo_job j = make_job( w, h, bd, numCand, lambda );
          EXPECT( geoHostJob( &j, org.get(), predPtr, ( int ) ( jobs & 1 ), res.get(), split.get(), blend.get() ) == 0 );
          jobs++;
          const vtmhip_geo_result &r = *res.get();
          for( int c = 0; c < VTMHIP_GEO_MAX_CAND; c++ )
          {
            EXPECT( ( c < numCand ) == ( r.sadWhole[c] != GEO_HOST_NO_COST ) );
            for( int s = 0; s < GEO_NUM_SPLIT; s++ )
              EXPECT( c < numCand ? split[s * VTMHIP_GEO_MAX_CAND + c] <= r.sadWhole[c] : split[s * VTMHIP_GEO_MAX_CAND + c] == GEO_HOST_NO_COST );
          }
          EXPECT( r.numPassed >= 0 && r.numPassed <= GEO_NUM_SPLIT * geoNumPairs( numCand ) && r.numTested == ( r.numPassed < 60 ? r.numPassed : 60 ) );
          regimes[r.numPassed == 0 ? 0 : r.numPassed <= 60 ? 1 : 2]++;
          const double best = geoBestWholeCost( r.sadWhole, numCand, lambda );
          for( int t = 0; t < VTMHIP_GEO_MAX_TRY; t++ )
          {
            const vtmhip_geo_combo &c = r.combo[t];
            if( t >= r.numTested )
            {
              EXPECT( c.dist == GEO_HOST_NO_COST && c.cost == 0.0 && c.splitDir == 0 && c.cand0 == 0 && c.cand1 == 0 );
              continue;
            }
            EXPECT( c.splitDir < GEO_NUM_SPLIT && c.cand0 < numCand && c.cand1 < numCand && c.cand0 != c.cand1 );
            const double c0 = geoSideCost( split[c.splitDir * VTMHIP_GEO_MAX_CAND + c.cand0], c.cand0, lambda );
            const double c1 = geoSideCost( r.sadWhole[c.cand1] - split[c.splitDir * VTMHIP_GEO_MAX_CAND + c.cand1], c.cand1, lambda );
            EXPECT( !( c0 + c1 > best ) && c.cost == c0 + c1 + 6.0 * lambda );
            if( t )
            {
              const vtmhip_geo_combo &p = r.combo[t - 1];
              EXPECT( p.cost < c.cost || ( p.cost == c.cost && ( p.splitDir < c.splitDir || ( p.splitDir == c.splitDir && pair_index( p.cand0, p.cand1 ) < pair_index( c.cand0, c.cand1 ) ) ) ) );
            }
            uint64_t       sad = 0;
            const int16_t *b = blend.get() + ( size_t ) t * w * h;
            for( int i = 0; i < w * h; i++ )
            {
              const int lo = geoRoundSample( pred[c.cand0][i], bd ), hi = geoRoundSample( pred[c.cand1][i], bd );
              EXPECT( b[i] >= ( lo < hi ? lo : hi ) - 1 && b[i] <= ( lo < hi ? hi : lo ) + 1 );
              sad += ( uint64_t ) abs( ( int ) org[i] - ( int ) b[i] );
            }
            if( !( ( jobs - 1 ) & 1 ) ) EXPECT( c.dist == sad );
            else EXPECT( c.dist != GEO_HOST_NO_COST );
          }
        }
    }
  EXPECT( regimes[0] > 0 && regimes[1] > 0 && regimes[2] > 0 );
  printf( "geo jobs: list regimes empty %d, short %d, capped %d\n", regimes[0], regimes[1], regimes[2] );
  return jobs;
}

static void check_ties()
{
  // duplicate candidates: equal costs must come out by splitDir, then by the pair order
  const int w = 16, h = 16, bd = 10;
  auto      org = heap<int16_t>( ( size_t ) w * h ), p0 = heap<int16_t>( ( size_t ) w * h );
  for( int i = 0; i < w * h; i++ ) { org[i] = ( int16_t ) ( ( i * 37 ) & 1023 ); p0[i] = ( int16_t ) ( ( ( ( i * 11 ) & 1023 ) << 4 ) - 8192 ); }
  const int16_t       *pred[VTMHIP_GEO_MAX_CAND] = { p0.get(), p0.get(), p0.get(), nullptr, nullptr, nullptr };
  const vtmhip_geo_job j = make_job( w, h, bd, 3, 0.0 );   // lambda 0: every combination costs the whole SAD
  auto                 res = heap<vtmhip_geo_result>( 1 );
  EXPECT( geoHostJob( &j, org.get(), pred, 1, res.get(), nullptr, nullptr ) == 0 );
  EXPECT( res[0].numPassed == GEO_NUM_SPLIT * 6 && res[0].numTested == 60 );
  for( int t = 0; t < 60; t++ )
  {
    int c0, c1;
    geoPair( t % 6, c0, c1 );
    EXPECT( res[0].combo[t].splitDir == t / 6 && res[0].combo[t].cand0 == c0 && res[0].combo[t].cand1 == c1 && res[0].combo[t].cost == ( double ) res[0].sadWhole[0] );
  }
}

static void check_predicate()
{
  const int w = 8, h = 8;
  auto      org = heap<int16_t>( ( size_t ) w * h ), p = heap<int16_t>( ( size_t ) w * h );
  const int16_t *pred[VTMHIP_GEO_MAX_CAND] = { p.get(), p.get(), p.get(), p.get(), p.get(), p.get() };
  auto      res = heap<vtmhip_geo_result>( 1 );
  int       bad = 0, good = 0;
  auto      run = [&]( const vtmhip_geo_job &j, bool ok )
  {
    memset( res.get(), 0x5a, sizeof( vtmhip_geo_result ) );
    const int st = geoHostJob( &j, org.get(), pred, 1, res.get(), nullptr, nullptr );
    EXPECT( ( st == 0 ) == ok );
    if( !ok )
    {
      const unsigned char *b = reinterpret_cast<const unsigned char *>( res.get() );
      for( size_t i = 0; i < sizeof( vtmhip_geo_result ); i++ ) EXPECT( b[i] == 0x5a );
      bad++;
    }
    else good++;
  };
  vtmhip_geo_job j;
  run( make_job( 8, 8, 8, 2, 0.0 ), true );
  run( make_job( 8, 8, 12, 6, 1.0e300 ), true );
  j = make_job( 8, 8, 10, 2, 1.0 ); j.width = 4; run( j, false );
  j = make_job( 8, 8, 10, 2, 1.0 ); j.width = 64; run( j, false );            // 64 x 8: w < 8h fails
  j = make_job( 8, 8, 10, 2, 1.0 ); j.height = 12; run( j, false );
  j = make_job( 8, 8, 10, 2, 1.0 ); j.bitDepth = 7; run( j, false );
  j = make_job( 8, 8, 10, 2, 1.0 ); j.bitDepth = 13; run( j, false );
  j = make_job( 8, 8, 10, 2, 1.0 ); j.numCand = 1; run( j, false );
  j = make_job( 8, 8, 10, 2, 1.0 ); j.numCand = 7; run( j, false );
  j = make_job( 8, 8, 10, 2, 1.0 ); j.orgStride = 7; run( j, false );
  j = make_job( 8, 8, 10, 2, 1.0 ); j.cand[1].refStride = 7; run( j, false );
  j = make_job( 8, 8, 10, 2, 1.0 ); j.cand[2].refStride = 7; run( j, true );   // beyond numCand: not read
  j = make_job( 8, 8, 10, 2, 1.0 ); j.sqrtLambda = -1.0; run( j, false );
  j = make_job( 8, 8, 10, 2, 1.0 ); j.sqrtLambda = std::numeric_limits<double>::infinity(); run( j, false );
  j = make_job( 8, 8, 10, 2, 1.0 ); j.sqrtLambda = std::numeric_limits<double>::quiet_NaN(); run( j, false );
  j = make_job( 8, 8, 10, 2, 1.0 ); j.cand[0].keepOff = 0;
  EXPECT( geoJobOk( j, 64, 64, true ) && !geoJobOk( j, 64, 64, false ) && !geoJobOk( make_job( 16, 16, 10, 2, 1.0 ), 8, 8, true ) );
  vtmhip_geo_cu_blend_job b = vtmhip_geo_cu_blend_job();
  b.width = 16; b.height = 8; b.bitDepth = 10; b.splitDir = 63; b.chroma = 1; b.src0Stride = b.src1Stride = b.dstStride = 8;
  EXPECT( geoBlendJobOk( b ) );
  b.dstStride = 7; EXPECT( !geoBlendJobOk( b ) ); b.dstStride = 8;
  b.splitDir = 64; EXPECT( !geoBlendJobOk( b ) ); b.splitDir = 0;
  b.chroma = 2; EXPECT( !geoBlendJobOk( b ) ); b.chroma = 0; EXPECT( !geoBlendJobOk( b ) );   // luma needs a stride of 16
  b.src0Stride = b.src1Stride = b.dstStride = 16; EXPECT( geoBlendJobOk( b ) );
  b.bitDepth = 13; EXPECT( !geoBlendJobOk( b ) ); b.bitDepth = 10;
  b.width = 64; EXPECT( !geoBlendJobOk( b ) );
  printf( "geo predicate: %d rejected, %d accepted\n", bad, good );
}

int main()
{
  std::mt19937 rng( 2026 );
  check_tables();
  const long jobs = check_jobs( rng );
  check_ties();
  check_predicate();
  printf( "geo rules: %ld jobs, %d failures\n", jobs, g_failures );
  return g_failures ? 1 : 0;
}
