// test_stage.cpp -- the HIP-free part of vtm_amd/csrc/stage.hpp (region planning, strided pack / unpack, the span of a stepped walk), exhaustively over small
// shapes.  Built with -fsanitize=address,undefined and run as its own process (tests/test_stage_cpp.py): an out-of-bounds copy or an overflow aborts it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../vtm_amd/csrc/stage.hpp"

static int failures = 0;
#define CHECK( cond )                                                          \
  do {                                                                         \
    if( !( cond ) ) { failures++; printf( "%s:%d: %s\n", __FILE__, __LINE__, #cond ); } \
  } while( 0 )

static const int WIDTHS[] = { 1, 2, 3, 5, 8, 127, 128 }, HEIGHTS[] = { 1, 2, 7, 128 }, EXTRA[] = { 0, 1, 3 }, STEPS[] = { -2, -1, 1, 2 };

// the layouts the entries plan: two or three blocks, a span, a job, a result slot -- every region aligned, inside the total, and disjoint from the others
static void test_regions( int w, int h )
{
  const size_t blk = ( size_t ) w * h * 2;
  const size_t sizes[] = { blk, blk, 1, ( size_t ) w * 2 + 1, 63, 64, 65, 56, 8, blk };
  StagePlan    p;
  std::vector<size_t> off;
  for( size_t s : sizes ) off.push_back( p.region( s ) );
  CHECK( p.total % StagePlan::ALIGN == 0 );
  for( size_t i = 0; i < off.size(); i++ )
  {
    CHECK( off[i] % StagePlan::ALIGN == 0 );
    CHECK( p.inside( off[i], sizes[i] ) );
    for( size_t k = 0; k < i; k++ ) CHECK( off[k] + sizes[k] <= off[i] );
  }
  CHECK( p.inside( 0, p.total ) && !p.inside( 0, p.total + 1 ) && !p.inside( p.total, 1 ) && !p.inside( p.total + 64, 0 ) && !p.inside( 64, ~( size_t ) 0 ) );
}

// pack followed by unpack: the identity inside the block, nothing outside it touched; also with a negative stride (rows stored bottom-up)
static void test_pack( int w, int h, int stride, bool negative )
{
  const size_t n = ( size_t ) stride * h;
  std::vector<int16_t> src( n ), dst( n, ( int16_t ) -21846 ), compact( ( size_t ) w * h + 2, ( int16_t ) 0x5555 );
  for( size_t i = 0; i < n; i++ ) src[i] = ( int16_t ) ( i * 31 + 7 );
  const ptrdiff_t  s  = negative ? -stride : stride;
  const ptrdiff_t  first = negative ? ( ptrdiff_t ) stride * ( h - 1 ) : 0;   // index of row 0
  stage_pack( compact.data() + 1, src.data() + first, s, w, h );
  CHECK( compact.front() == 0x5555 && compact.back() == 0x5555 );
  for( int y = 0; y < h; y++ )
    for( int x = 0; x < w; x++ ) CHECK( compact[1 + ( size_t ) y * w + x] == src[first + y * s + x] );
  stage_unpack( dst.data() + first, s, compact.data() + 1, w, h );
  for( int y = 0; y < h; y++ )
    for( int x = 0; x < stride; x++ )
    {
      const ptrdiff_t i = first + y * s + x;
      CHECK( dst[i] == ( x < w ? src[i] : ( int16_t ) -21846 ) );
    }
}

static void test_span( int w, int rows, long stepX, long rowStep )
{
  long lo = 0, hi = 0;
  for( int r = 0; r < rows; r++ )
    for( int x = 0; x < w; x++ )
    {
      const long o = r * rowStep + x * stepX;
      lo = o < lo ? o : lo; hi = o > hi ? o : hi;
    }
  const StageSpan s = stage_walk_span( w, rows, stepX, rowStep );
  CHECK( s.lo == lo && s.hi == hi && s.count() == ( size_t ) ( hi - lo + 1 ) );
}

int main()
{
  for( int w : WIDTHS )
    for( int h : HEIGHTS )
    {
      test_regions( w, h );
      for( int e : EXTRA )
      {
        test_pack( w, h, w + e, false );
        test_pack( w, h, w + e, true );
        for( int step : STEPS )
          for( int sign : { 1, -1 } )
          {
            test_span( w, h, step, ( long ) sign * ( w + e ) );                       // weightedGeoBlk: rowStep = weightStride
            test_span( w, h, step, ( long ) w * step + ( long ) sign * ( w + e ) );   // xGetSADwMask: rowStep = width * stepX + maskStride
          }
      }
    }
  printf( "%d failures\n", failures );
  return failures ? 1 : 0;
}
