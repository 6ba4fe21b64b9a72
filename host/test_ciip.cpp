// test_ciip.cpp -- the CIIP rules of vtm_amd/csrc/ciip_rules.hpp and the host entries' bodies of ciip_host.hpp (both HIP-free) as a stand-alone program under
// AddressSanitizer and UBSan (tests/test_ciip_cpp.py builds and runs it).  Every CIIP size, every weight, 8 .. 12 bit, with and without the LUT steps: the lines, the
// original, the inter blocks, the LUTs and the outputs sit in heap arrays of exactly their length, so a read or write past one is a report.  Every index a prediction
// reads a line at goes through INTRA_LINE_CHECK, which counts the ones outside [0, 2W] / [0, 2H] and marks the ones it sees: the filtered lines must have been formed
// from every sample of both lines.  What the entries leave is checked for what can be said without a second implementation: the blend inside the sample range and
// between its two inputs, flat inputs blended exactly, the SAD equal to the one recomputed from the outputs, a zero SATD exactly for a block equal to the original,
// UINT64_MAX beyond numCand; then the predicate's edge jobs: each malformed field rejected with nothing written, each edge value accepted.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <random>

static long g_lineReads = 0, g_lineOutside = 0;
static bool g_seen[2 * 64 + 2];
#define INTRA_LINE_CHECK( idx, last ) \
  do { g_lineReads++; if( ( idx ) < 0 || ( idx ) > ( last ) ) g_lineOutside++; else g_seen[idx] = true; } while( 0 )

#include "../vtm_amd/csrc/ciip_host.hpp"

static int g_failures = 0;
#define EXPECT( cond ) do { if( !( cond ) ) { g_failures++; if( g_failures < 20 ) printf( "FAIL %s:%d %s\n", __FILE__, __LINE__, #cond ); } } while( 0 )

template<class T> static std::unique_ptr<T[]> heap( size_t n ) { return std::unique_ptr<T[]>( new T[n]() ); }

static const int SIDES[5] = { 4, 8, 16, 32, 64 };

static vtmhip_ciip_job make_job( int w, int h, int bd, int numCand )
{
  vtmhip_ciip_job j = vtmhip_ciip_job();
  j.width = ( int16_t ) w; j.height = ( int16_t ) h; j.bitDepth = ( uint8_t ) bd; j.numCand = ( uint8_t ) numCand; j.orgStride = w;
  for( int k = 0; k < VTMHIP_CIIP_MAX_CAND; k++ )
  {
    j.cand[k].mode = ( uint8_t ) ( k % 4 ); j.cand[k].refStride[0] = j.cand[k].refStride[1] = w; j.cand[k].srcStride = w; j.cand[k].keepOff = -1;
  }
  return j;
}

static long check_blocks( std::mt19937 &rng )
{
  long blocks = 0;
  for( int wi = 0; wi < 5; wi++ )
    for( int hi = 0; hi < 5; hi++ )
    {
      const int w = SIDES[wi], h = SIDES[hi];
      if( !ciipSizeOk( w, h ) ) continue;
      for( int bd = 8; bd <= 12; bd++ )
        for( int flags = 0; flags < 4; flags++ )
        {
          const int  maxVal = ( 1 << bd ) - 1, nLine = 2 * w + 2 * h + 2, numCand = 1 + ( int ) ( rng() % 4 );
          const bool lmcs = ( flags + bd ) % 2 != 0, flat = rng() % 5 == 0;
          auto lines = heap<int16_t>( nLine ), org = heap<int16_t>( ( size_t ) w * h ), blend = heap<int16_t>( ( size_t ) numCand * w * h );
          auto fwd = heap<int16_t>( ( size_t ) maxVal + 1 ), inv = heap<int16_t>( ( size_t ) maxVal + 1 );
          auto satd = heap<uint64_t>( VTMHIP_CIIP_MAX_CAND ), sad = heap<uint64_t>( VTMHIP_CIIP_MAX_CAND );
          std::unique_ptr<int16_t[]> inter[VTMHIP_CIIP_MAX_CAND];
          const int16_t             *interPtr[VTMHIP_CIIP_MAX_CAND] = { nullptr, nullptr, nullptr, nullptr };
          const int flatLine = ( int ) ( rng() % ( maxVal + 1 ) ), flatInter = ( int ) ( rng() % ( maxVal + 1 ) );
          for( int i = 0; i < nLine; i++ ) lines[i] = ( int16_t ) ( flat ? flatLine : rng() % ( maxVal + 1 ) );
          lines[2 * w + 1] = lines[0];
          for( int i = 0; i < w * h; i++ ) org[i] = ( int16_t ) ( rng() % ( maxVal + 1 ) );
          for( int i = 0; i <= maxVal; i++ ) { fwd[i] = ( int16_t ) ( maxVal - i ); inv[i] = ( int16_t ) ( maxVal - i ); }   // an involution: inv( fwd( v ) ) = v
          for( int k = 0; k < numCand; k++ )
          {
            inter[k] = heap<int16_t>( ( size_t ) w * h );
            for( int i = 0; i < w * h; i++ ) inter[k][i] = ( int16_t ) ( flat ? flatInter : rng() % ( maxVal + 1 ) );
            interPtr[k] = inter[k].get();
          }
          vtmhip_ciip_job j = make_job( w, h, bd, numCand );
          j.leftIntra = ( uint8_t ) ( flags & 1 ); j.aboveIntra = ( uint8_t ) ( flags >> 1 ); j.lmcs = lmcs;
          memset( g_seen, 0, sizeof( g_seen ) );
          EXPECT( ciipHostJob( &j, lines.get(), org.get(), interPtr, lmcs ? fwd.get() : nullptr, lmcs ? inv.get() : nullptr, blend.get(), satd.get(), sad.get() ) == 0 );
          // the [1 2 1] filter has read every sample of the longer line's range on both lines
          for( int i = 0; i <= 2 * ( w < h ? w : h ); i++ ) EXPECT( g_seen[i] );
          const int wIntra = ciipWeightIntra( j.leftIntra, j.aboveIntra );
          EXPECT( wIntra == 1 + ( flags & 1 ) + ( flags >> 1 ) );
          for( int k = 0; k < VTMHIP_CIIP_MAX_CAND; k++ )
          {
            if( k >= numCand ) { EXPECT( satd[k] == CIIP_HOST_NO_COST && sad[k] == CIIP_HOST_NO_COST ); continue; }
            uint64_t mySad = 0;
            for( int i = 0; i < w * h; i++ )
            {
              const int v = blend[( size_t ) k * w * h + i];
              EXPECT( v >= 0 && v <= maxVal );
              if( flat ) EXPECT( v == ciipBlendSample( lmcs ? maxVal - flatInter : flatInter, flatLine, wIntra ) );   // planar and PDPC of flat lines are flat
              const int seen = lmcs ? inv[v] : v;
              mySad += ( uint64_t ) abs( ( int ) org[i] - seen );
            }
            EXPECT( mySad == sad[k] );
            EXPECT( satd[k] != CIIP_HOST_NO_COST && ( satd[k] == 0 ) == ( sad[k] == 0 ) );
          }
          // the block the distortion sees as the original: both costs are zero
          {
            auto same = heap<int16_t>( ( size_t ) w * h );
            for( int i = 0; i < w * h; i++ ) same[i] = lmcs ? inv[blend[i]] : blend[i];
            uint64_t a = 1, b = 1;
            ciipHostCosts( same.get(), w, same.get(), w, h, a, b );
            EXPECT( a == 0 && b == 0 );
          }
          blocks++;
          // the chroma block of this CU through the blend entry, in place inside a rim
          const int cw = w / 2, ch = h / 2;
          vtmhip_ciip_blend_job bj = vtmhip_ciip_blend_job();
          bj.width = ( int16_t ) cw; bj.height = ( int16_t ) ch; bj.bitDepth = ( uint8_t ) bd; bj.chroma = 1; bj.leftIntra = j.leftIntra; bj.aboveIntra = j.aboveIntra;
          bj.predStride = cw + 3; bj.predOff = bj.predStride + 1;
          const size_t planeN = ( size_t ) ( ch + 2 ) * ( cw + 3 );
          auto plane = heap<int16_t>( planeN ), before = heap<int16_t>( planeN ), cl = heap<int16_t>( 2 * cw + 2 * ch + 2 );
          for( size_t i = 0; i < planeN; i++ ) before[i] = plane[i] = ( int16_t ) ( rng() % ( maxVal + 1 ) );
          for( int i = 0; i < 2 * cw + 2 * ch + 2; i++ ) cl[i] = ( int16_t ) ( rng() % ( maxVal + 1 ) );
          const int st = ciipHostBlendJob( &bj, cl.get(), plane.get(), nullptr );
          EXPECT( ( st == 0 ) == ( cw > 2 ) );
          for( int y = 0; y < ch + 2; y++ )
            for( int x = 0; x < cw + 3; x++ )
            {
              const bool inside = st == 0 && y >= 1 && y <= ch && x >= 1 && x <= cw;
              const int  v = plane[y * ( cw + 3 ) + x];
              if( !inside ) EXPECT( v == before[y * ( cw + 3 ) + x] );
              else EXPECT( v >= 0 && v <= maxVal );
            }
        }
    }
  return blocks;
}

static void check_rules()
{
  for( int w = 4; w <= 128; w <<= 1 )
    for( int h = 4; h <= 128; h <<= 1 ) EXPECT( ciipSizeOk( w, h ) == ( w * h >= 64 && w < 128 && h < 128 ) );
  EXPECT( !ciipSizeOk( 12, 12 ) && !ciipSizeOk( 0, 64 ) && !ciipSizeOk( -8, -8 ) && !ciipSizeOk( 2, 32 ) );
  EXPECT( ciipWeightIntra( 0, 0 ) == 1 && ciipWeightIntra( 1, 0 ) == 2 && ciipWeightIntra( 0, 1 ) == 2 && ciipWeightIntra( 1, 1 ) == 3 && ciipWeightIntra( 255, 7 ) == 3 );
  const int nc[8] = { 0, 0, 1, 2, 3, 4, 4, 4 };
  for( int n = -1; n <= 6; n++ ) EXPECT( ciipNumCand( n ) == nc[n + 1] );
  for( int bd = 8; bd <= 12; bd += 4 )
  {
    const int mx = ( 1 << bd ) - 1;
    for( int wI = 1; wI <= 3; wI++ )
    {
      EXPECT( ciipBlendSample( 0, 0, wI ) == 0 && ciipBlendSample( mx, mx, wI ) == mx );
      EXPECT( ciipBlendSample( mx, 0, wI ) == ( ( 4 - wI ) * mx + 2 ) >> 2 && ciipBlendSample( 0, mx, wI ) == ( wI * mx + 2 ) >> 2 );
    }
  }
  EXPECT( ciipChromaSizeOk( 8, 2 ) && ciipChromaSizeOk( 32, 2 ) && ciipChromaSizeOk( 4, 4 ) && ciipChromaSizeOk( 32, 32 ) );
  EXPECT( !ciipChromaSizeOk( 2, 8 ) && !ciipChromaSizeOk( 2, 32 ) && !ciipChromaSizeOk( 4, 2 ) && !ciipChromaSizeOk( 64, 4 ) && !ciipChromaSizeOk( 8, 64 ) );
}

// the predicate's edge jobs through the host entry: a rejected job writes nothing
static void check_predicate()
{
  const int w = 16, h = 4, n = w * h;
  auto lines = heap<int16_t>( 2 * w + 2 * h + 2 ), org = heap<int16_t>( n ), lut = heap<int16_t>( 1 << 12 );
  auto i0 = heap<int16_t>( n ), i1 = heap<int16_t>( n ), i2 = heap<int16_t>( n ), i3 = heap<int16_t>( n );
  const int16_t *inter[4] = { i0.get(), i1.get(), i2.get(), i3.get() };
  auto run = [&]( const vtmhip_ciip_job &j, bool luts, int wOut, int hOut ) {
    auto     blend = heap<int16_t>( ( size_t ) 4 * wOut * hOut );
    uint64_t satd[4] = { 7, 7, 7, 7 }, sad[4] = { 7, 7, 7, 7 };
    for( int i = 0; i < 4 * wOut * hOut; i++ ) blend[i] = 0x1234;
    const int st = ciipHostJob( &j, lines.get(), org.get(), inter, luts ? lut.get() : nullptr, luts ? lut.get() : nullptr, blend.get(), satd, sad );
    if( st != 0 )
    {
      for( int i = 0; i < 4 * wOut * hOut; i++ ) EXPECT( blend[i] == 0x1234 );
      for( int k = 0; k < 4; k++ ) EXPECT( satd[k] == 7 && sad[k] == 7 );
    }
    return st;
  };
  const vtmhip_ciip_job good = make_job( w, h, 10, 4 );
  EXPECT( run( good, false, w, h ) == 0 );
#define REJECT( change ) do { vtmhip_ciip_job m = good; change; EXPECT( run( m, false, w, h ) != 0 ); } while( 0 )
#define ACCEPT( change ) do { vtmhip_ciip_job m = good; change; EXPECT( run( m, false, w, h ) == 0 ); } while( 0 )
  REJECT( m.width = 4; m.height = 8 ); REJECT( m.width = 128 ); REJECT( m.height = 128 ); REJECT( m.width = 12 ); REJECT( m.width = 0 ); REJECT( m.height = -4 );
  REJECT( m.bitDepth = 7 ); REJECT( m.bitDepth = 13 ); ACCEPT( m.bitDepth = 8 ); ACCEPT( m.bitDepth = 12 );
  REJECT( m.numCand = 0 ); REJECT( m.numCand = 5 ); REJECT( m.numCand = 255 ); ACCEPT( m.numCand = 1 );
  REJECT( m.orgStride = w - 1 ); REJECT( m.orgStride = -w );
  REJECT( m.cand[2].mode = 4 ); REJECT( m.cand[0].mode = 255 );
  ACCEPT( m.numCand = 2; m.cand[3].mode = 9 );                      // beyond numCand: not looked at
  REJECT( m.cand[3].srcStride = w - 1 ); ACCEPT( m.cand[0].srcStride = 0 );   // the given stride counts for mode 3 alone
  REJECT( m.cand[0].refStride[0] = w - 1 ); ACCEPT( m.cand[0].refStride[1] = 0 );   // list 0
  REJECT( m.cand[1].refStride[1] = w - 1 ); ACCEPT( m.cand[1].refStride[0] = 0 );   // list 1
  REJECT( m.cand[2].refStride[0] = 0 ); REJECT( m.cand[2].refStride[1] = 0 );       // bi
  REJECT( m.lmcs = 1 );                                             // no LUTs in the call
#undef REJECT
#undef ACCEPT
  vtmhip_ciip_job m = good;
  m.lmcs = 1;
  EXPECT( run( m, true, w, h ) == 0 );
  // the size above the entry's 64 x 64 limit never reaches the output arrays
  m = make_job( 128, 64, 10, 1 );
  EXPECT( run( m, false, 1, 1 ) != 0 );
  // null pointers
  uint64_t a[4], b[4];
  auto     out = heap<int16_t>( ( size_t ) 4 * n );
  EXPECT( ciipHostJob( nullptr, lines.get(), org.get(), inter, nullptr, nullptr, out.get(), a, b ) != 0 );
  EXPECT( ciipHostJob( &good, nullptr, org.get(), inter, nullptr, nullptr, out.get(), a, b ) != 0 );
  const int16_t *holes[4] = { i0.get(), nullptr, i2.get(), i3.get() };
  EXPECT( ciipHostJob( &good, lines.get(), org.get(), holes, nullptr, nullptr, out.get(), a, b ) != 0 );
  // the blend entry's edges
  vtmhip_ciip_blend_job bj = vtmhip_ciip_blend_job();
  bj.width = 8; bj.height = 8; bj.bitDepth = 10; bj.predStride = 8;
  EXPECT( ciipBlendJobOk( bj, 0 ) && ciipBlendJobOk( bj, 10 ) );
  bj.mapFwd = 1;
  EXPECT( !ciipBlendJobOk( bj, 0 ) && !ciipBlendJobOk( bj, 8 ) && ciipBlendJobOk( bj, 10 ) );
  bj.chroma = 1;
  EXPECT( !ciipBlendJobOk( bj, 10 ) );
  bj.mapFwd = 0; bj.predStride = 7;
  EXPECT( !ciipBlendJobOk( bj, 10 ) );
}

int main()
{
  std::mt19937 rng( 2026 );
  const long   blocks = check_blocks( rng );
  check_rules();
  check_predicate();
  EXPECT( g_lineReads > 0 && g_lineOutside == 0 );
  printf( "ciip rules: %ld blocks, %ld line reads, %ld outside, %d failures\n", blocks, g_lineReads, g_lineOutside, g_failures );
  return g_failures ? 1 : 0;
}
