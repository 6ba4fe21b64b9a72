// test_host_wp.cpp -- explicit weighted prediction through the host mirror (vtmhip_host.hpp): DistParam::applyWeight on the SAD / HAD / SSE / SSE_WTD slots,
// routed to the device by RdCost::setDeviceWeightedPrediction( true ), with wpCur set the way InterSearch::setWpScalingDistParam sets it
// (InterSearch.cpp:6057-6098).  Input file (little endian): int32 nCases; per case: int32 kind (0 SAD, 1 HAD, 2 SSE, 3 SSE_WTD), width, height, bitDepth,
// isBiPred, compID, w, offset, shift, round; uint64 maxDist; int16 org[h][w], cur[h][w].
// Prints one distortion per case, then "refused-when-off" when the installer is switched off again and the SAD slot refuses applyWeight, and
// "sse-subshift-check" when SSEw rejects a nonzero subShift (the reference's CHECK).  tests/test_gpu_wp.py builds and checks it.
#include <cstdio>
#include <string>
#include <vector>

#include "vtmhip_host.hpp"

using namespace vtmhip;

template<class T> static bool rd( FILE *f, T *p, size_t n ) { return fread( p, sizeof( T ), n, f ) == n; }

int main( int argc, char **argv )
{
  if( argc < 2 ) return 1;
  FILE *f = fopen( argv[1], "rb" );
  if( !f ) return 1;
  try
  {
    RdCost rdCost;
    RdCost::setDeviceWeightedPrediction( true );
    int32_t n = 0;
    if( !rd( f, &n, 1 ) ) return 1;
    for( int i = 0; i < n; i++ )
    {
      int32_t  c[10];
      uint64_t maxDist;
      if( !rd( f, c, 10 ) || !rd( f, &maxDist, 1 ) ) return 1;
      const int w = c[1], h = c[2];
      std::vector<Pel> org( ( size_t ) w * h ), cur( ( size_t ) w * h );
      if( !rd( f, org.data(), org.size() ) || !rd( f, cur.data(), cur.size() ) ) return 1;
      WPScalingParam wp[MAX_NUM_COMPONENT];
      const ComponentID comp = ( ComponentID ) c[5];
      wp[comp].w = c[6]; wp[comp].offset = c[7]; wp[comp].shift = c[8]; wp[comp].round = c[9];
      DistParam dp;
      const CPelBuf orgBuf( org.data(), w, w, h );
      if( c[0] <= 1 ) rdCost.setDistParam( dp, orgBuf, cur.data(), w, c[3], comp, 0, 1, c[0] == 1 );   // the motion-estimation slots
      else
      {
        dp.org = orgBuf; dp.cur = CPelBuf( cur.data(), w, w, h ); dp.bitDepth = c[3]; dp.compID = comp;
        const bool p2 = ( w & ( w - 1 ) ) == 0;
        dp.distFunc = RdCost::distFuncAt( ( c[0] == 2 ? DF_SSE : DF_SSE_WTD ) + ( p2 ? floorLog2( w ) : 0 ) );
      }
      dp.applyWeight = true; dp.isBiPred = c[4] != 0; dp.wpCur = wp;
      dp.maximumDistortionForEarlyExit = maxDist;
      printf( "%llu\n", ( unsigned long long ) dp.distFunc( dp ) );
    }
    Pel            s[16] = {};
    WPScalingParam wp[MAX_NUM_COMPONENT];
    wp[0].w = 1;
    DistParam dp;
    dp.org = dp.cur = CPelBuf( s, 4, 4, 4 );
    dp.compID = COMPONENT_Y; dp.bitDepth = 10; dp.applyWeight = true; dp.wpCur = wp; dp.subShift = 1;
    try { RdCost::distFuncAt( DF_SSE4 )( dp ); }
    catch( const Exception &e ) { if( std::string( e.what() ).find( "Subshift" ) != std::string::npos ) printf( "sse-subshift-check\n" ); }
    RdCost::setDeviceWeightedPrediction( false );
    dp.subShift = 0;
    try { RdCost::distFuncAt( DF_SAD4 )( dp ); }
    catch( const Exception &e ) { if( std::string( e.what() ).find( "applyWeight" ) != std::string::npos ) printf( "refused-when-off\n" ); }
  }
  catch( const Exception &e )
  {
    printf( "%s\n", e.what() );
    return 2;
  }
  fclose( f );
  return 0;
}
