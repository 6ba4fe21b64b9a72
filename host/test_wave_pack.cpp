// test_wave_pack.cpp -- the HIP-free part of vtm_amd/csrc/wave_pack.hpp (FastDiv, the item cursor, the group indexing and the launch rules) on the host.
// Built with -fsanitize=address,undefined and run as its own process (tests/test_wave_pack_cpp.py): a cursor that reads past ends[] or an overflow aborts it.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "../vtm_amd/csrc/wave_pack.hpp"

static int failures = 0;
#define CHECK( cond )                                                          \
  do {                                                                         \
    if( !( cond ) ) { failures++; printf( "%s:%d: %s\n", __FILE__, __LINE__, #cond ); } \
  } while( 0 )

static unsigned rngState = 12345u;
static unsigned rnd() { rngState = rngState * 1664525u + 1013904223u; return rngState >> 8; }

// every divisor the callers form (segments / tiles per row, block width: 1..128) against every index up to one row past 128 rows
static void test_fastdiv()
{
  for( int d = 1; d <= 128; d++ )
  {
    const FastDiv div( d );
    CHECK( div.d == d );
    for( int p = 0; p <= 128 * d + d; p++ )
      if( div( p ) != p / d ) { CHECK( div( p ) == p / d ); return; }
  }
}

// one group: counts[] items per job (0: rejected).  Every item t, walked lane-strided and in wave-uniform steps of 64 as the kernels do, must come out in the
// job whose [start, end) holds it, with the right local index, exactly once.  ends[] has exactly G entries: reading ends[G] is a heap overflow.
static void test_group( const std::vector<int> &counts )
{
  const int        G = ( int ) counts.size();
  std::vector<int> ends( G ), jobOf;
  int              total = 0;
  for( int j = 0; j < G; j++ )
  {
    for( int i = 0; i < counts[j]; i++ ) jobOf.push_back( j );
    ends[j] = total += counts[j];
  }
  for( int stepped = 0; stepped < 2; stepped++ )
  {
    std::vector<int> seen( total, 0 );
    for( int lane = 0; lane < 64; lane++ )
    {
      WaveCursor cur;
      auto       item = [&]( int t )
      {
        if( cur.beyond( t ) ) cur.advance( t, ends.data() );
        CHECK( cur.cj >= 0 && cur.cj < G && cur.cj == jobOf[t] );
        CHECK( cur.end == ends[cur.cj] && cur.start == ends[cur.cj] - counts[cur.cj] && t >= cur.start && t < cur.end );
        seen[t]++;
      };
      if( stepped )
        for( int b = 0; b < total; b += 64 ) { if( b + lane < total ) item( b + lane ); }
      else
        for( int t = lane; t < total; t += 64 ) item( t );
    }
    for( int t = 0; t < total; t++ ) CHECK( seen[t] == 1 );
  }
}

static int test_cursor()
{
  std::set<std::pair<int, int>> cases;   // (G, position of the forced zero)
  int below = 0, above = 0;
  for( int G = 1; G <= 64; G++ )
    for( int pos = 0; pos < 3; pos++ )
      for( int big = 0; big < 2; big++ )
      {
        std::vector<int> counts( G );
        // small: the whole group stays below 64 items; big: rows of segments up to 128 x 32, most of them small blocks
        for( int &c : counts ) c = big ? ( rnd() % 8 == 0 ? ( int ) ( rnd() % 4097 ) : ( int ) ( rnd() % 70 ) ) : ( int ) ( rnd() % ( 63 / G + 1 ) );
        for( int &c : counts )
          if( rnd() % 5 == 0 ) c = 0;
        counts[pos == 0 ? 0 : pos == 1 ? G / 2 : G - 1] = 0;
        if( big && G > 1 ) counts[pos == 0 ? G - 1 : 0] = 64 + ( int ) ( rnd() % 200 );   // a job that spans steps next to the rejected ones
        int total = 0;
        for( int c : counts ) total += c;
        ( total < 64 ? below : above )++;
        test_group( counts );
        cases.insert( { G, pos } );
      }
  CHECK( below >= 64 && above >= 64 );
  test_group( std::vector<int>( 64, 128 * 32 ) );   // the largest group: 64 blocks of 128 x 128
  test_group( std::vector<int>( 64, 1 ) );
  return ( int ) cases.size();
}

// the launch a batch of n jobs gets: every job belongs to exactly one (workgroup, round, wave, lane), inside the caps
static void test_launch( int numCUs, int n, int waves, int perCU )
{
  const int G = wave_jobs_per_wave( numCUs, n );
  CHECK( G >= 1 && G <= 64 );
  CHECK( G == 1 || ( long ) G * numCUs * 32 <= n );              // packing still leaves 32 waves per CU
  CHECK( G == 64 || ( long ) ( G + 1 ) * numCUs * 32 > n );      // and no looser than that allows
  const int nGroups = wave_groups( n, G ), blocks = wave_blocks( n, G, waves, numCUs * perCU );
  CHECK( ( long ) nGroups * G >= n && ( long ) ( nGroups - 1 ) * G < n );
  CHECK( blocks >= 1 && blocks <= numCUs * perCU && ( long ) ( blocks - 1 ) * waves < nGroups );
  CHECK( blocks == numCUs * perCU || ( long ) blocks * waves >= nGroups );
  std::vector<char> seen( n, 0 );
  for( int blk = 0; blk < blocks; blk++ )
    for( int round = blk * waves; round < nGroups; round += blocks * waves )   // the kernels' round loop
      for( int wv = 0; wv < waves; wv++ )
        for( int lane = 0; lane < 64; lane++ )
        {
          const WaveGroup g( round, wv, lane, n, G, nGroups );
          if( !g.mine ) continue;
          CHECK( g.job >= 0 && g.job < n && g.base == g.grp * G && g.job == g.base + lane );
          if( g.job >= 0 && g.job < n ) seen[g.job]++;
        }
  for( int i = 0; i < n; i++ )
    if( seen[i] != 1 ) { CHECK( seen[i] == 1 ); break; }
}

int main()
{
  test_fastdiv();
  const int cases = test_cursor();
  printf( "%d cursor cases (G, zero position)\n", cases );
  CHECK( cases >= 64 * 3 );
  for( int numCUs : { 1, 8, 256, 304 } )
  {
    const int unit = numCUs * 32;
    CHECK( wave_jobs_per_wave( numCUs, 1 ) == 1 && wave_jobs_per_wave( numCUs, unit - 1 ) == 1 && wave_jobs_per_wave( numCUs, unit ) == 1 );
    CHECK( wave_jobs_per_wave( numCUs, 2 * unit - 1 ) == 1 && wave_jobs_per_wave( numCUs, 2 * unit ) == 2 );
    CHECK( wave_jobs_per_wave( numCUs, 64 * unit - 1 ) == 63 && wave_jobs_per_wave( numCUs, 64 * unit ) == 64 && wave_jobs_per_wave( numCUs, 200 * unit ) == 64 );
    for( int perCU : { 8, 64 } )
      for( int n : { 1, 2, 3, 63, 64, 65, unit - 1, unit, unit + 1, 2 * unit - 1, 2 * unit, 2 * unit + 1, 3 * unit + 7, 64 * unit - 1, 64 * unit, 64 * unit + 1,
                     4 * perCU * numCUs * 64 + 5 } )   // the last: more groups than the cap's workgroups hold, the kernels loop
        test_launch( numCUs, n, 4, perCU );
  }
  CHECK( wave_blocks( 1000000, 1, 4, 2048 ) == 2048 && wave_blocks( 8192, 1, 4, 2048 ) == 2048 && wave_blocks( 8188, 1, 4, 2048 ) == 2047 );
  printf( "%d failures\n", failures );
  return failures ? 1 : 0;
}
