// test_mip.cpp -- vtm_amd/csrc/mip_rules.hpp (the matrix-based intra prediction rules: shape, reduced boundaries, the matrix product, the closed-form up-sampling)
// compiled for the host.  Built with -fsanitize=address,undefined and run as its own process (tests/test_mip_cpp.py).  A few hand-computed cases, then every
// (shape, mode, transposed) with the lines in heap arrays of exactly W + 1 and H + 1 samples and the matrices in heap arrays of exactly their size, filled with
// seeded random bytes (the rules do not depend on the trained values): MIP_LINE_CHECK sees the index of every read before it happens and counts the ones outside
// [1, W] / [1, H]; an overrun would also abort under ASan.  Mode k transposed on W x H must equal the transpose of mode k on H x W with the lines swapped where the
// block is up-sampled in at most one direction -- with two directions the two 1-D passes round in a different order, and the identity is not asserted there.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static long g_reads = 0, g_outside = 0;
#define MIP_LINE_CHECK( idx, last ) \
  do { g_reads++; if( ( idx ) < 1 || ( idx ) > ( last ) ) g_outside++; } while( 0 )

#include "../vtm_amd/csrc/mip_rules.hpp"

static int failures = 0;
#define CHECK( cond )                                                          \
  do {                                                                         \
    if( !( cond ) ) { failures++; printf( "%s:%d: %s\n", __FILE__, __LINE__, #cond ); } \
  } while( 0 )

static const int SIDES[] = { 4, 8, 16, 32, 64 };

static unsigned long long rngState = 88172645463325252ull;
static unsigned long long rnd() { rngState ^= rngState << 13; rngState ^= rngState >> 7; rngState ^= rngState << 17; return rngState; }

struct Matrices
{
  std::vector<uint8_t> m4, m8, m16;   // exact sizes
  explicit Matrices( int fill ) : m4( MIP_BYTES_4X4 ), m8( MIP_BYTES_8X8 ), m16( MIP_BYTES_16X16 )
  {
    for( auto *m : { &m4, &m8, &m16 } )
      for( auto &v : *m ) v = ( uint8_t ) ( fill < 0 ? rnd() & 255 : fill );
  }
};

static std::vector<int16_t> predict( int w, int h, int bd, int mode, int t, const std::vector<int16_t> &top, const std::vector<int16_t> &left, const Matrices &M )
{
  std::vector<int16_t> out( ( size_t ) w * h );
  mipPredict( w, h, bd, mode, t, top.data(), left.data(), M.m4.data(), M.m8.data(), M.m16.data(), out.data() );
  return out;
}

static void test_by_hand()
{
  CHECK( mipSizeId( 4, 4 ) == 0 && mipSizeId( 4, 8 ) == 1 && mipSizeId( 64, 4 ) == 1 && mipSizeId( 8, 8 ) == 1 && mipSizeId( 8, 16 ) == 2 && mipSizeId( 64, 64 ) == 2 );
  CHECK( mipNumModes( 0 ) == 16 && mipNumModes( 1 ) == 8 && mipNumModes( 2 ) == 6 );
  MipShape s = mipShape( 64, 4 );
  CHECK( s.sizeId == 1 && s.bdry == 4 && s.pred == 4 && s.upH == 16 && s.upV == 1 && s.log2UpH == 4 && s.log2UpV == 0 );
  s = mipShape( 32, 64 );
  CHECK( s.sizeId == 2 && s.bdry == 4 && s.pred == 8 && s.upH == 4 && s.upV == 8 );
  s = mipShape( 4, 4 );
  CHECK( s.bdry == 2 && s.pred == 4 && s.upH == 1 && s.upV == 1 );

  // 4 x 4, 10 bit: reduced top { 110, 150 }, reduced left { 70, 30 }.  With every weight 32 the product cancels against the offset and every entry is the input
  // offset; 64 more on the weight of input 1 in one row adds exactly in[1] there: 150 - 110 = 40 (top | left), 30 - 70 = -40 (left | top).
  const std::vector<int16_t> top = { 0x7fff, 100, 120, 140, 160 }, left = { 0x7fff, 80, 60, 40, 20 };
  CHECK( mipBoundarySample( top.data(), 4, 2, 0 ) == 110 && mipBoundarySample( top.data(), 4, 2, 1 ) == 150 && mipBoundarySample( left.data(), 4, 2, 1 ) == 30 );
  const int a[2] = { 110, 150 }, b[2] = { 70, 30 };
  CHECK( mipInputAt( s, 10, a, b, 0 ) == 512 - 110 && mipInputAt( s, 10, a, b, 1 ) == 40 && mipInputAt( s, 10, a, b, 2 ) == -40 && mipInputAt( s, 10, a, b, 3 ) == -80 );
  Matrices M( 32 );
  const int mode = 3;
  M.m4[( mode * 16 + 6 ) * 4 + 1] = 96;   // row 6 = entry (1, 2) of the 4 x 4 result
  std::vector<int16_t> v = predict( 4, 4, 10, mode, 0, top, left, M );
  for( int i = 0; i < 16; i++ ) CHECK( v[i] == ( i == 6 ? 150 : 110 ) );
  v = predict( 4, 4, 10, mode, 1, top, left, M );
  for( int i = 0; i < 16; i++ ) CHECK( v[i] == ( i == 9 ? 30 : 70 ) );   // transposed: entry (1, 2) lands at (2, 1)
  v = predict( 4, 4, 10, mode + 1, 0, top, left, M );
  for( int i = 0; i < 16; i++ ) CHECK( v[i] == 110 );
  M.m4[( mode * 16 + 6 ) * 4 + 1] = 255;   // 223 * 40 / 64 = 139.4: 110 + 139
  v = predict( 4, 4, 10, mode, 0, top, left, M );
  CHECK( v[6] == 249 );
  v = predict( 4, 4, 8, mode, 0, top, left, M );   // 8 bit: in[0] changes, the weights of 32 still cancel it; 249 stays below 255
  CHECK( v[6] == 249 && v[0] == 110 );

  // a constant boundary and weights of 32: the input offset everywhere, through both up-sampling passes
  const Matrices N( 32 );
  for( int w : SIDES )
    for( int h : SIDES )
    {
      const std::vector<int16_t> t( w + 1, 300 ), l( h + 1, 300 );
      for( int tr = 0; tr < 2; tr++ )
      {
        v = predict( w, h, 10, mipNumModes( mipSizeId( w, h ) ) - 1, tr, t, l, N );
        bool all = true;
        for( int16_t x : v ) all &= x == 300;
        CHECK( all );
      }
    }

  // 8 x 4: horizontal factor 2.  Reduced block 200 everywhere (top | left, top constant 200), left 100: column 0 is the rounded mean with the left neighbour
  {
    const std::vector<int16_t> t( 9, 200 ), l( 5, 100 );
    v = predict( 8, 4, 10, 0, 0, t, l, N );
    for( int y = 0; y < 4; y++ ) CHECK( v[y * 8] == 150 && v[y * 8 + 1] == 200 && v[y * 8 + 2] == 200 && v[y * 8 + 7] == 200 );
  }
  // 4 x 8 transposed: vertical factor 2.  Reduced block 200 (left | top, left constant 200), top 101: row 0 is ( 101 + 200 + 1 ) >> 1
  {
    const std::vector<int16_t> t( 5, 101 ), l( 9, 200 );
    v = predict( 4, 8, 10, 0, 1, t, l, N );
    for( int x = 0; x < 4; x++ ) CHECK( v[x] == 151 && v[4 + x] == 200 && v[8 + x] == 200 && v[28 + x] == 200 );
  }
  // 16 x 4: factor 4 from the left neighbour 100 towards 200: 125, 150, 175, 200
  {
    const std::vector<int16_t> t( 17, 200 ), l( 5, 100 );
    v = predict( 16, 4, 10, 0, 0, t, l, N );
    CHECK( v[0] == 125 && v[1] == 150 && v[2] == 175 && v[3] == 200 && v[4] == 200 );
  }
}

static void test_grid()
{
  const Matrices M( -1 );
  long jobs = 0, mirrored = 0, twoWayDiffers = 0, twoWay = 0;
  for( int w : SIDES )
    for( int h : SIDES )
      for( int bd = 8; bd <= 12; bd += 2 )
      {
        const int maxVal = ( 1 << bd ) - 1;
        std::vector<int16_t> top( w + 1 ), left( h + 1 );   // exact sizes; index 0 is never read
        for( auto &v : top ) v = ( int16_t ) ( rnd() % ( maxVal + 1 ) );
        for( auto &v : left ) v = ( int16_t ) ( rnd() % ( maxVal + 1 ) );
        top[0] = left[0] = 0x7fff;
        const MipShape s = mipShape( w, h );
        CHECK( mipBlockOk( w, h, bd, 0 ) && s.upH * s.pred == w && s.upV * s.pred == h );
        for( int mode = 0; mode < mipNumModes( s.sizeId ); mode++ )
          for( int t = 0; t < 2; t++ )
          {
            CHECK( mipJobOk( s, mode, t ) );
            const std::vector<int16_t> a = predict( w, h, bd, mode, t, top, left, M );
            const std::vector<int16_t> m = predict( h, w, bd, mode, !t, left, top, M );
            bool same = true, inRange = true;
            for( int y = 0; y < h; y++ )
              for( int x = 0; x < w; x++ )
              {
                same &= a[( size_t ) y * w + x] == m[( size_t ) x * h + y];
                inRange &= a[( size_t ) y * w + x] >= 0 && a[( size_t ) y * w + x] <= maxVal;
              }
            CHECK( inRange );
            if( s.upH == 1 || s.upV == 1 ) { CHECK( same ); mirrored++; }
            else { twoWay++; twoWayDiffers += !same; }
            jobs++;
          }
      }
  CHECK( g_outside == 0 );
  CHECK( mirrored > 0 && twoWayDiffers > 0 );   // the identity holds where it is true and only there
  printf( "%ld jobs, %ld line reads, %ld outside their line, %ld mirrored, %ld of %ld two-way jobs differ from their mirror\n", jobs, g_reads, g_outside, mirrored, twoWayDiffers,
          twoWay );
}

static void test_entry_checks()
{
  CHECK( !mipBlockOk( 128, 4, 10, 0 ) && !mipBlockOk( 4, 2, 10, 0 ) && !mipBlockOk( 12, 8, 10, 0 ) && !mipBlockOk( 8, 8, 7, 0 ) && !mipBlockOk( 8, 8, 13, 0 ) &&
         !mipBlockOk( 8, 8, 10, 1 ) && mipBlockOk( 64, 4, 12, 0 ) );
  CHECK( !mipJobOk( mipShape( 4, 4 ), 16, 0 ) && mipJobOk( mipShape( 4, 4 ), 15, 1 ) && !mipJobOk( mipShape( 8, 8 ), 8, 0 ) && !mipJobOk( mipShape( 16, 16 ), 6, 0 ) &&
         !mipJobOk( mipShape( 16, 16 ), 0, 2 ) && !mipJobOk( mipShape( 16, 16 ), -1, 0 ) );
}

int main()
{
  test_by_hand();
  test_grid();
  test_entry_checks();
  printf( "%d failures\n", failures );
  return failures ? 1 : 0;
}
