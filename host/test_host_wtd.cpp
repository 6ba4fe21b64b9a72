// test_host_wtd.cpp -- the DF_SSE_WTD slots of the host mirror (vtmhip_host.hpp) driven the way the reference's callers drive them:
// RdCost::getDistPart( org, cur, bitDepth, compID, DF_SSE_WTD, &orgLuma ) (RdCost.cpp:411-455).  Input file (little endian):
//   int32 lumaBD, signalType; double chromaWeight, distortionWeight[Cb], distortionWeight[Cr]; double lut[1 << lumaBD]; int32 nCases;
//   per case: int32 width, height, compID, chromaFormat, lumaWidth, lumaHeight; int16 org[h][w], cur[h][w], orgLuma[lumaHeight][lumaWidth]
// Prints one distortion per case, then "applyWeight-fallback-ok" when the applyWeight guard refuses the device path.  tests/test_gpu_dist_wtd.py builds and checks it.
#include <cstdio>
#include <vector>

#include "vtmhip_host.hpp"

using namespace vtmhip;
static_assert( DF_SSE_WTD == DF_SAD_WITH_MASK + 1 && DF_SSE16N_WTD + 1 == DF_TOTAL_FUNCTIONS, "the WTD slots follow every earlier slot" );

template<class T> static bool rd( FILE *f, T *p, size_t n ) { return fread( p, sizeof( T ), n, f ) == n; }

int main( int argc, char **argv )
{
  if( argc < 2 ) return 1;
  FILE *f = fopen( argv[1], "rb" );
  if( !f ) return 1;
  try
  {
    RdCost  rdCost;
    int32_t hdr[2];
    double  wts[3];
    if( !rd( f, hdr, 2 ) || !rd( f, wts, 3 ) ) return 1;
    std::vector<double> lut( ( size_t ) 1 << hdr[0] );
    int32_t             n = 0;
    if( !rd( f, lut.data(), lut.size() ) || !rd( f, &n, 1 ) ) return 1;
    check( vtmhip_set_luma_level_weights( context(), lut.data(), hdr[0], hdr[1], wts[0], nullptr ), "vtmhip_set_luma_level_weights" );
    rdCost.setDistortionWeight( COMPONENT_Cb, wts[1] );
    rdCost.setDistortionWeight( COMPONENT_Cr, wts[2] );
    for( int i = 0; i < n; i++ )
    {
      int32_t c[6];
      if( !rd( f, c, 6 ) ) return 1;
      const int        w = c[0], h = c[1];
      const ComponentID comp = ( ComponentID ) c[2];
      std::vector<Pel> org( ( size_t ) w * h ), cur( ( size_t ) w * h ), luma( ( size_t ) c[4] * c[5] );
      if( !rd( f, org.data(), org.size() ) || !rd( f, cur.data(), cur.size() ) || !rd( f, luma.data(), luma.size() ) ) return 1;
      rdCost.setChromaFormat( ( ChromaFormat ) c[3] );
      const CPelBuf orgBuf( org.data(), w, w, h ), curBuf( cur.data(), w, w, h ), lumaBuf( luma.data(), c[4], c[4], c[5] );
      const Distortion d = rdCost.getDistPart( orgBuf, curBuf, hdr[0], comp, DF_SSE_WTD, comp == COMPONENT_Y ? &orgBuf : &lumaBuf );
      printf( "%llu\n", ( unsigned long long ) d );
    }
    // explicit weighted prediction stays with the scalar RdCostWeightPrediction::xGetSSEw: the trampoline refuses it
    Pel       s[16] = {};
    DistParam dp;
    dp.org = dp.cur = dp.orgLuma = CPelBuf( s, 4, 4, 4 );
    dp.compID = COMPONENT_Y; dp.applyWeight = true;
    try { RdCost::distFuncAt( DF_SSE4_WTD )( dp ); }
    catch( const Exception &e ) { if( std::string( e.what() ).find( "applyWeight" ) != std::string::npos ) printf( "applyWeight-fallback-ok\n" ); }
  }
  catch( const Exception &e )
  {
    printf( "%s\n", e.what() );
    return 2;
  }
  fclose( f );
  return 0;
}
