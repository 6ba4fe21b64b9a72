// test_intra.cpp -- vtm_amd/csrc/intra_rules.hpp (the luma intra prediction rules: parameters, filtered lines, the per-sample formulas of planar, DC and the
// angular modes with their PDPC) compiled for the host.  Built with -fsanitize=address,undefined and run as its own process (tests/test_intra_cpp.py).  A few
// hand-computed cases, then every (shape, mode, multiRefIdx) with the lines in heap arrays of exactly 2W + 1 + m and 2H + 1 + m samples: INTRA_LINE_CHECK sees the
// index of every read before it happens and counts the ones outside [0, 2W + m] / [0, 2H + m]; an overrun would also abort under ASan.  The transposed block with
// the mirrored mode (68 - mode, lines swapped) must give the transposed prediction.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static long g_reads = 0, g_outside = 0;
#define INTRA_LINE_CHECK( idx, last ) \
  do { g_reads++; if( ( idx ) < 0 || ( idx ) > ( last ) ) g_outside++; } while( 0 )

#include "../vtm_amd/csrc/chroma_taps.hpp"
#include "../vtm_amd/csrc/intra_rules.hpp"

static int failures = 0;
#define CHECK( cond )                                                          \
  do {                                                                         \
    if( !( cond ) ) { failures++; printf( "%s:%d: %s\n", __FILE__, __LINE__, #cond ); } \
  } while( 0 )

static const int16_t CUBIC[32][4] = { VTMHIP_CHROMA_FILTER_TAPS };
static const int     SIDES[] = { 4, 8, 16, 32, 64 };

static unsigned long long rngState = 88172645463325252ull;
static unsigned long long rnd() { rngState ^= rngState << 13; rngState ^= rngState >> 7; rngState ^= rngState << 17; return rngState; }

struct Lines
{
  std::vector<int16_t> top, left, fTop, fLeft;   // exact sizes
  Lines( int w, int h, int m, int maxVal ) : top( 2 * w + 1 + m ), left( 2 * h + 1 + m ), fTop( 2 * w + 1 + m ), fLeft( 2 * h + 1 + m )
  {
    for( auto &v : top ) v = ( int16_t ) ( rnd() % ( maxVal + 1 ) );
    for( auto &v : left ) v = ( int16_t ) ( rnd() % ( maxVal + 1 ) );
    left[0] = top[0];
    filter( w, h, m );
  }
  void filter( int w, int h, int m )
  {
    if( m ) return;
    for( int i = 0; i <= 2 * w; i++ ) fTop[i] = intraFilteredSample( top.data(), left.data(), i, 2 * w );
    for( int i = 0; i <= 2 * h; i++ ) fLeft[i] = intraFilteredSample( left.data(), top.data(), i, 2 * h );
  }
};

static std::vector<int16_t> predict( const Lines &ln, int w, int h, int mode, int m, int bd )
{
  vtmhip_intra_params p;
  intraPredParams( w, h, mode, m, p );
  IntraBlk b;
  b.top = p.refFilterFlag ? ln.fTop.data() : ln.top.data();
  b.left = p.refFilterFlag ? ln.fLeft.data() : ln.left.data();
  b.w = w; b.h = h; b.log2W = intraLog2( w ); b.log2H = intraLog2( h ); b.m = m; b.maxVal = ( 1 << bd ) - 1;
  IntraBlk u = b;
  u.top = ln.top.data(); u.left = ln.left.data();
  const int dc = intraDcVal( u );
  std::vector<int16_t> out( ( size_t ) w * h );
  for( int y = 0; y < h; y++ )
    for( int x = 0; x < w; x++ ) out[( size_t ) y * w + x] = intraPredSample( p, mode, b, dc, CUBIC, x, y );
  return out;
}

static void test_by_hand()
{
  vtmhip_intra_params p;
  intraPredParams( 4, 4, 2, 0, p );   // no wide angle on a square: horizontal, angle 32
  CHECK( p.predMode == 2 && !p.isModeVer && p.intraPredAngle == 32 && p.invAngle == 512 && p.angularScale == 0 && p.applyPDPC && !p.refFilterFlag && !p.interpolationFlag );
  intraPredParams( 8, 4, 2, 0, p );   // 2 : 1 moves modes 2 .. 7 to 67 .. 72
  CHECK( p.predMode == 67 && p.isModeVer && p.intraPredAngle == 35 && p.invAngle == 468 && p.angularScale == 0 && p.applyPDPC && !p.refFilterFlag && !p.interpolationFlag );
  intraPredParams( 8, 4, 8, 0, p );
  CHECK( p.predMode == 8 );
  intraPredParams( 4, 8, 61, 0, p );
  CHECK( p.predMode == -4 && !p.isModeVer && p.intraPredAngle == 64 );
  intraPredParams( 4, 8, 60, 0, p );
  CHECK( p.predMode == 60 );
  intraPredParams( 16, 16, 34, 0, p );   // the diagonal: integer slope, filtered lines, no PDPC
  CHECK( p.predMode == 34 && p.isModeVer && p.intraPredAngle == -32 && p.invAngle == 512 && !p.applyPDPC && p.refFilterFlag && !p.interpolationFlag );
  intraPredParams( 16, 16, 36, 0, p );   // fractional slope past the threshold of 2: smoothing taps
  CHECK( p.intraPredAngle == -26 && !p.refFilterFlag && p.interpolationFlag );
  intraPredParams( 16, 16, 36, 1, p );   // no filter of either kind and no PDPC off line 0
  CHECK( !p.refFilterFlag && !p.interpolationFlag && !p.applyPDPC );
  intraPredParams( 16, 16, 52, 0, p );   // |52 - 50| = 2 is not above the threshold
  CHECK( !p.refFilterFlag && !p.interpolationFlag );
  intraPredParams( 16, 16, 53, 0, p );
  CHECK( p.interpolationFlag );
  intraPredParams( 8, 8, 0, 0, p );
  CHECK( p.refFilterFlag && p.applyPDPC );
  intraPredParams( 4, 8, 0, 0, p );
  CHECK( !p.refFilterFlag );
  intraPredParams( 8, 8, 1, 0, p );
  CHECK( !p.refFilterFlag && p.applyPDPC );
  intraPredParams( 4, 64, 66, 0, p );   // 66 is moved on a tall block: predMode 1 is not vertical
  CHECK( p.predMode == 1 && !p.isModeVer );

  Lines ln( 4, 4, 0, 1023 );
  const int16_t top[9] = { 100, 110, 120, 130, 140, 150, 160, 170, 180 }, left[9] = { 100, 90, 80, 70, 60, 50, 40, 30, 20 };
  memcpy( ln.top.data(), top, sizeof top );
  memcpy( ln.left.data(), left, sizeof left );
  ln.filter( 4, 4, 0 );
  CHECK( ln.fTop[0] == 100 && ln.fLeft[0] == 100 && ln.fTop[1] == 110 && ln.fTop[8] == 180 && ln.fLeft[1] == 90 && ln.fLeft[8] == 20 );
  std::vector<int16_t> v = predict( ln, 4, 4, 50, 0, 10 );   // pure vertical: the column above plus the clipped PDPC, weights 32, 8, 2
  CHECK( v[0] == 105 && v[1] == 119 && v[2] == 130 && v[3] == 140 );
  v = predict( ln, 4, 4, 1, 0, 10 );   // the DC value of these lines: ( 500 + 300 + 4 ) >> 3 = 100, PDPC at (0, 0): 100 + ( ( 32 * -10 + 32 * 10 + 32 ) >> 6 )
  CHECK( v[0] == 100 && v[15] == 100 );
  v = predict( ln, 4, 4, 0, 0, 10 );   // planar (0, 0): hor 420, vert 380 -> ( 1680 + 1520 + 16 ) >> 5 = 100; PDPC adds ( 32 * -10 + 32 * 10 + 32 ) >> 6 = 0
  CHECK( v[0] == 100 );
  v = predict( ln, 4, 4, 66, 0, 10 );  // angle 32: top[x + y + 2], then the PDPC column from left[x + y + 2]: 120 + ( ( 32 * ( 80 - 120 ) + 32 ) >> 6 ) = 100
  CHECK( v[0] == 100 && v[3] == 150 && v[15] == 180 );   // (3, 3) would be top[8] = 180, the last sample
  v = predict( ln, 4, 4, 34, 0, 10 );  // angle -32: the diagonal through the corner; (0, 1) comes from the side line: left[1]
  CHECK( v[0] == 100 && v[5] == 100 && v[1] == 110 && v[4] == 90 );
}

static void test_grid()
{
  long clamped = 0;
  for( int w : SIDES )
    for( int h : SIDES )
      for( int m = 0; m <= INTRA_MAX_MRL; m++ )
      {
        const int bd = 8 + 2 * m;
        Lines ln( w, h, m, ( 1 << bd ) - 1 ), lnT( h, w, m, ( 1 << bd ) - 1 );
        lnT.top = ln.left; lnT.left = ln.top;
        lnT.filter( h, w, m );
        CHECK( intraBlockOk( w, h, bd, m ) );
        for( int mode = 0; mode < INTRA_NUM_LUMA_MODE; mode++ )
        {
          CHECK( intraModeOk( mode, m ) == !( mode == 0 && m ) );
          if( !intraModeOk( mode, m ) ) continue;
          vtmhip_intra_params p;
          intraPredParams( w, h, mode, m, p );
          CHECK( p.predMode >= -14 && p.predMode <= 80 && ( p.refFilterFlag + p.interpolationFlag ) <= 1 && p.angularScale >= -8 && p.angularScale <= 2 );
          if( m ) CHECK( !p.applyPDPC && !p.refFilterFlag && !p.interpolationFlag );
          if( p.applyPDPC && mode > INTRA_DC ) CHECK( p.intraPredAngle >= 0 && p.angularScale >= 0 );
          if( w * h <= 32 ) CHECK( !p.refFilterFlag && !p.interpolationFlag );
          const std::vector<int16_t> a = predict( ln, w, h, mode, m, bd );
          const int mirror = mode <= INTRA_DC ? mode : 68 - mode;
          const std::vector<int16_t> t = predict( lnT, h, w, mirror, m, bd );
          bool same = true, inRange = true;
          for( int y = 0; y < h; y++ )
            for( int x = 0; x < w; x++ )
            {
              same &= a[( size_t ) y * w + x] == t[( size_t ) x * h + y];
              inRange &= a[( size_t ) y * w + x] >= 0 && a[( size_t ) y * w + x] < ( 1 << bd );
            }
          CHECK( same );
          CHECK( inRange );   // random lines inside the bit depth: the cubic taps' overshoot is clipped, everything else is an average
          // how often the replication rule acts: reads of the main line past its last sample
          if( p.intraPredAngle > 0 )
          {
            const int mainSize = p.isModeVer ? w : h, rows = p.isModeVer ? h : w;
            for( int r = 0; r < rows; r++ )
              if( m + ( ( p.intraPredAngle * ( r + 1 + m ) ) >> 5 ) + mainSize - 1 + 3 > 2 * mainSize + m ) clamped++;
          }
        }
      }
  CHECK( g_outside == 0 );
  CHECK( clamped > 0 );
  printf( "%ld line reads, %ld outside their line, %ld rows reach past the main line's last sample\n", g_reads, g_outside, clamped );
}

static void test_entry_checks()
{
  CHECK( !intraBlockOk( 128, 4, 10, 0 ) && !intraBlockOk( 4, 2, 10, 0 ) && !intraBlockOk( 12, 8, 10, 0 ) && !intraBlockOk( 8, 8, 7, 0 ) && !intraBlockOk( 8, 8, 13, 0 ) &&
         !intraBlockOk( 8, 8, 10, 3 ) );
  CHECK( !intraModeOk( 67, 0 ) && !intraModeOk( 255, 0 ) && !intraModeOk( 0, 1 ) && intraModeOk( 1, 2 ) && intraModeOk( 66, 2 ) );
}

int main()
{
  test_by_hand();
  test_grid();
  test_entry_checks();
  printf( "%d failures\n", failures );
  return failures ? 1 : 0;
}
