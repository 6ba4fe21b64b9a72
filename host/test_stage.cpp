// test_stage.cpp -- the HIP-free part of vtm_amd/csrc/stage.hpp (region planning at both alignments, strided pack / unpack, the span of a stepped walk),
// exhaustively over small shapes; and the eight device workspace layouts planned at 256 bytes against the offsets their call sites used to compute by hand.  Built with -fsanitize=address,undefined and run as its own process (tests/test_stage_cpp.py): an out-of-bounds copy or an overflow aborts it.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <vector>

#include "../include/vtmhip.h"
#include "../vtm_amd/csrc/stage.hpp"

static int failures = 0;
#define CHECK( cond )                                                          \
  do {                                                                         \
    if( !( cond ) ) { failures++; printf( "%s:%d: %s\n", __FILE__, __LINE__, #cond ); } \
  } while( 0 )

static const int WIDTHS[] = { 1, 2, 3, 5, 8, 127, 128 }, HEIGHTS[] = { 1, 2, 7, 128 }, EXTRA[] = { 0, 1, 3 }, STEPS[] = { -2, -1, 1, 2 };

// the layouts the entries plan: two or three blocks, a span, a job, a result slot -- every region aligned, inside the total, and disjoint from the others
template<class Plan>
static void test_regions( int w, int h )
{
  const size_t blk = ( size_t ) w * h * 2;
  const size_t sizes[] = { blk, blk, 1, ( size_t ) w * 2 + 1, 63, 64, 65, 56, 8, 255, 256, 257, blk };
  Plan         p;
  std::vector<size_t> off;
  for( size_t s : sizes ) off.push_back( p.region( s ) );
  CHECK( p.total % Plan::ALIGN == 0 );
  for( size_t i = 0; i < off.size(); i++ )
  {
    CHECK( off[i] % Plan::ALIGN == 0 );
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

// ---- the device workspaces: WorkRegions against the hand formulas of the eight call sites, record sizes as in include/vtmhip.h ------------------------------
static size_t A( size_t v ) { return ( v + 255 ) & ~( size_t ) 255; }
enum : size_t { S_INT = 4, S_TU_JOB = 40, S_TU_RES = 16, S_LFNST_JOB = 40, S_JCCR_JOB = 48, S_JCCR_RES = 32, S_TZ_JOB = 208, S_FULL_JOB = 72, S_ME_RES = 32, S_FRAC_JOB = 56,
              S_FRAC_RES = 16, S_DIST_JOB = 32, S_ME_JOB = 232, S_ME_OUT = 48, S_TZ_SAVED = 64, S_U64 = 8, REFINE_SLOTS = 18 };
static_assert( sizeof( vtmhip_tu_job ) == S_TU_JOB && sizeof( vtmhip_tu_result ) == S_TU_RES && sizeof( vtmhip_lfnst_chain_job ) == S_LFNST_JOB &&
                   sizeof( vtmhip_jccr_job ) == S_JCCR_JOB && sizeof( vtmhip_jccr_result ) == S_JCCR_RES && sizeof( vtmhip_tz_job ) == S_TZ_JOB &&
                   sizeof( vtmhip_full_job ) == S_FULL_JOB && sizeof( vtmhip_me_result ) == S_ME_RES && sizeof( vtmhip_frac_job ) == S_FRAC_JOB &&
                   sizeof( vtmhip_frac_result ) == S_FRAC_RES && sizeof( vtmhip_dist_job ) == S_DIST_JOB && sizeof( vtmhip_me_job ) == S_ME_JOB &&
                   sizeof( vtmhip_me_out ) == S_ME_OUT,
               "record sizes" );   // (S_TZ_SAVED: me.hip's TzSaved, a Range and twelve words)
static const size_t COUNTS[] = { 0, 1, 15, 16, 17, 64, 1000 };

// plans `sizes` in order and checks every offset and the total
static void check_layout( std::initializer_list<size_t> sizes, std::initializer_list<size_t> want, size_t wantTotal )
{
  WorkRegions p;
  auto        w = want.begin();
  for( size_t s : sizes ) CHECK( p.region( s ) == *w++ );
  CHECK( p.total == A( wantTotal ) );
}

static void test_work_layouts( size_t n, size_t m )
{
  {   // intra_chain.hip: n plain + m LFNST jobs -- block index, expanded jobs, results, the LFNST chain's jobs
    const size_t all = n + m, oJobs = A( all * S_INT ), oRes = A( oJobs + all * S_TU_JOB ), oLf = A( oRes + all * S_TU_RES );
    check_layout( { all * S_INT, all * S_TU_JOB, all * S_TU_RES, m * S_LFNST_JOB }, { 0, oJobs, oRes, oLf }, oLf + m * S_LFNST_JOB );
  }
  {   // intra_chroma_chain.hip: n single + m joint jobs
    const size_t oJBlk = A( n * S_INT ), oXTu = A( oJBlk + m * S_INT ), oXJoint = A( oXTu + n * S_TU_JOB ), oTuRes = A( oXJoint + m * S_JCCR_JOB ),
                 oJRes = A( oTuRes + n * S_TU_RES );
    check_layout( { n * S_INT, m * S_INT, n * S_TU_JOB, m * S_JCCR_JOB, n * S_TU_RES, m * S_JCCR_RES }, { 0, oJBlk, oXTu, oXJoint, oTuRes, oJRes }, oJRes + m * S_JCCR_RES );
  }
  {   // sbt.hip: n candidates, m sub-TUs -- the cursor in the first 256 bytes
    const size_t oIdx = 256, oJobs = A( oIdx + 3 * n * S_INT ), oRes = A( oJobs + m * S_TU_JOB );
    check_layout( { S_INT, 3 * n * S_INT, m * S_TU_JOB, m * S_TU_RES }, { 0, oIdx, oJobs, oRes }, oRes + m * S_TU_RES );
  }
  for( int flags = 0; flags < 16; flags++ )   // mest.hip: the regions a uniform batch never touches are empty; 256 bytes of slack at the end
  {
    const bool   direct = flags & 1, allBi = flags & 2, allUni = flags & 4, needDist = flags & 8;
    const size_t slot = ( m + 4 ) * 8 * sizeof( int16_t );   // a block of ( m + 4 ) x 8 samples
    size_t off = 0;
    const size_t oPattern = off; off = A( off + ( direct ? 0 : n * slot ) );
    const size_t oTz      = off; off = A( off + ( allBi ? 0 : n * S_TZ_JOB ) );
    const size_t oFull    = off; off = A( off + ( allUni ? 0 : n * S_FULL_JOB ) );
    const size_t oIres    = off; off = A( off + n * S_ME_RES );
    const size_t oFrac    = off; off = A( off + n * S_FRAC_JOB );
    const size_t oFres    = off; off = A( off + n * S_FRAC_RES );
    const size_t oDist    = off; off = A( off + ( needDist ? n * REFINE_SLOTS * S_DIST_JOB : 0 ) );
    const size_t oDout    = off; off = A( off + ( needDist ? n * REFINE_SLOTS * S_U64 : 0 ) );
    check_layout( { direct ? 0 : n * slot, allBi ? 0 : n * S_TZ_JOB, allUni ? 0 : n * S_FULL_JOB, n * S_ME_RES, n * S_FRAC_JOB, n * S_FRAC_RES,
                    needDist ? n * REFINE_SLOTS * S_DIST_JOB : 0, needDist ? n * REFINE_SLOTS * S_U64 : 0, 256 },
                  { oPattern, oTz, oFull, oIres, oFrac, oFres, oDist, oDout, off }, off + 256 );
  }
  // pis.hip, both sites: the two SADs of every row
  check_layout( { 2 * n * S_U64 }, { 0 }, A( 2 * n * S_U64 ) );
  check_layout( { 2 * n * S_U64 }, { 0 }, A( 2 * n * S_U64 ) );
  for( int tu = 0; tu < 2; tu++ )   // bucket.hpp for the ME rows and for the TU chain: three tables of 20 ints at the head
  {
    const size_t job = tu ? S_TU_JOB : S_ME_JOB, res = tu ? S_TU_RES : S_ME_OUT, oJobs = 256, oRes = A( oJobs + n * job ), oPerm = A( oRes + n * res );
    check_layout( { 3 * 20 * S_INT, n * job, n * res, n * S_INT }, { 0, oJobs, oRes, oPerm }, oPerm + n * S_INT );
  }
  for( int parts = 0; parts < 2; parts++ )   // me.hip's split scan: saved states, the scan list with its counter, the totals right behind it
  {
    const size_t totBytes = parts ? n * ( 40 * 40 + 1 ) * sizeof( unsigned ) : 0, oList = A( n * S_TZ_SAVED ), oTot = A( oList + ( n + 1 ) * S_INT );
    check_layout( { n * S_TZ_SAVED, ( n + 1 ) * S_INT, totBytes }, { 0, oList, oTot }, oTot + totBytes );
  }
}

// an empty region takes the offset of the region behind it and overlaps nothing before it
static void test_empty_region()
{
  for( size_t first : { 1, 100, 256, 257 } )
  {
    WorkRegions  p;
    const size_t a = p.region( first ), z = p.region( 0 ), b = p.region( 8 );
    CHECK( a == 0 && z >= a + first && b == z && p.inside( z, 0 ) && p.inside( b, 8 ) && p.total == b + 256 );
  }
}

int main()
{
  for( size_t n : COUNTS )
    for( size_t m : COUNTS ) test_work_layouts( n, m );
  test_empty_region();
  for( int w : WIDTHS )
    for( int h : HEIGHTS )
    {
      test_regions<StagePlan>( w, h );
      test_regions<WorkRegions>( w, h );
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
