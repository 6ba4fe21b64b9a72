// test_sbt.cpp -- vtm_amd/csrc/sbt_rules.hpp (the SBT rules, the combination step of calcMinDistSbt and the RD-cost skip) compiled for the host, walked over every
// CU size and mode.  Built with -fsanitize=address,undefined and run as its own process (tests/test_sbt_cpp.py): an out-of-bounds index into the partition or
// estimate tables, a shift out of range or a signed overflow aborts it.  The skip rule is exercised as sbtSkipByRdCost from the header; the exported wrapper
// vtmhip_sbt_skip_by_rdcost (sbt.hip: three lines, the NULL / sbtIdx / sbtPos checks in front of the same call) needs the HIP library and is covered by
// tests/test_sbt.py through the C ABI.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../vtm_amd/csrc/sbt_rules.hpp"

static int failures = 0;
#define CHECK( cond )                                                          \
  do {                                                                         \
    if( !( cond ) ) { failures++; printf( "%s:%d: %s\n", __FILE__, __LINE__, #cond ); } \
  } while( 0 )

static const int SIDES[] = { 4, 8, 16, 32, 64 };

static unsigned long long rngState = 88172645463325252ull;
static unsigned long long rnd() { rngState ^= rngState << 13; rngState ^= rngState >> 7; rngState ^= rngState << 17; return rngState; }

// the tiles of a mode: the coded tile and the other position's tile cover the block along the split side without overlap (half modes), the coded tile lies inside
// the block (all modes); the transform pair is DCT-2 on every side above 32
static void test_tiles( int w, int h )
{
  const int allowed = sbtAllowed( w, h, 64 );
  CHECK( sbtAllowed( w, h, 32 ) == ( w > 32 || h > 32 ? 0 : allowed ) );
  CHECK( ( allowed & 1 ) == 0 && allowed < ( 1 << NUMBER_SBT_IDX ) );
  CHECK( numSbtModeRdo( allowed ) <= 2 * SBT_NUM_RDO );
  for( int mode = 0; mode < NUMBER_SBT_MODE; mode++ )
  {
    const int idx = getSbtIdxFromSbtMode( mode ), pos = getSbtPosFromSbtMode( mode );
    CHECK( getSbtMode( idx, pos ) == mode );
    if( !targetSbtAllowed( idx, allowed ) ) continue;
    for( int c = 0; c < 2; c++ )
    {
      const int cw = c ? w / 2 : w, ch = c ? h / 2 : h;
      int x, y, tw, th, x2, y2, tw2, th2;
      sbtCodedTile( cw, ch, idx, pos, x, y, tw, th );
      sbtCodedTile( cw, ch, idx, 1 - pos, x2, y2, tw2, th2 );
      CHECK( x >= 0 && y >= 0 && tw >= 2 && th >= 2 && x + tw <= cw && y + th <= ch );
      CHECK( ( tw & ( tw - 1 ) ) == 0 && ( th & ( th - 1 ) ) == 0 );
      std::vector<unsigned char> cover( ( size_t ) cw * ch, 0 );
      for( int yy = y; yy < y + th; yy++ ) for( int xx = x; xx < x + tw; xx++ ) cover[( size_t ) yy * cw + xx]++;
      for( int yy = y2; yy < y2 + th2; yy++ ) for( int xx = x2; xx < x2 + tw2; xx++ ) cover[( size_t ) yy * cw + xx]++;
      int twice = 0, none = 0;
      for( unsigned char v : cover ) { twice += v == 2; none += v == 0; }
      CHECK( twice == 0 && none == ( idx >= SBT_VER_QUAD ? cw * ch / 2 : 0 ) );
      if( c == 0 )
      {
        int th_ = -1, tv_ = -1;
        sbtTrTypes( idx, pos, tw, th, th_, tv_ );
        CHECK( th_ >= SBT_TR_DCT2 && th_ <= SBT_TR_DST7 && tv_ >= SBT_TR_DCT2 && tv_ <= SBT_TR_DST7 );
        if( tw > 32 || th > 32 ) CHECK( th_ == SBT_TR_DCT2 && tv_ == SBT_TR_DCT2 );
        else CHECK( th_ != SBT_TR_DCT2 && tv_ != SBT_TR_DCT2 && ( pos == SBT_POS1 ? th_ == SBT_TR_DST7 && tv_ == SBT_TR_DST7 : ( th_ == SBT_TR_DCT8 ) != ( tv_ == SBT_TR_DCT8 ) ) );
      }
    }
  }
}

// the combination step and the skip rule on random partition tables of this CU size, every allowed-mask subset of the size's mask
static void test_combine( int w, int h )
{
  const int npx = sbtNumPart( w ), npy = sbtNumPart( h ), full = sbtAllowed( w, h, 64 );
  for( int trial = 0; trial < 64; trial++ )
  {
    const int allowed = full & ( int ) rnd();
    uint64_t  dist[4][4];
    memset( dist, 0, sizeof( dist ) );
    uint64_t total = 0;
    for( int j = 0; j < npy; j++ )
      for( int i = 0; i < npx; i++ ) { dist[j][i] = rnd() % ( trial & 1 ? 4292870401ull * 2 : 5000 ); total += dist[j][i]; }
    uint64_t est[9];
    uint8_t  order[8];
    const double distScale = trial % 3 == 0 ? 1.0 / 57.3 : 4.0;
    const int    skipAll   = sbtCombine( dist, npx, npy, allowed, distScale, est, order );
    CHECK( est[8] == total && skipAll == ( distScale * double( total ) < double( 12 << 15 ) ) );
    int tried = 0;
    for( int m = 0; m < NUMBER_SBT_MODE; m++ )
    {
      const bool on = !skipAll && targetSbtAllowed( getSbtIdxFromSbtMode( m ), allowed );
      CHECK( on ? est[m] <= total : est[m] == ~( uint64_t ) 0 );
      tried += order[m] != 255;
    }
    CHECK( tried == ( skipAll ? 0 : numSbtModeRdo( allowed ) ) );
    for( int k = 0; k < NUMBER_SBT_MODE; k++ )
    {
      if( order[k] == 255 ) continue;
      CHECK( order[k] < NUMBER_SBT_MODE && est[order[k]] != ~( uint64_t ) 0 );
      for( int k2 = 0; k2 < k; k2++ ) CHECK( order[k2] != order[k] );
      if( k && order[k - 1] != 255 && ( order[k - 1] < SBT_VER_Q0 ) == ( order[k] < SBT_VER_Q0 ) )
        CHECK( est[order[k - 1]] < est[order[k]] || ( est[order[k - 1]] == est[order[k]] && order[k - 1] < order[k] ) );
    }
    for( int m = 0; m < NUMBER_SBT_MODE; m++ )
    {
      const int idx = getSbtIdxFromSbtMode( m ), pos = getSbtPosFromSbtMode( m );
      const double best = distScale * double( est[m] ) * ( trial & 2 ? 0.5 : 3.0 ) + 400000.0;
      for( int root = 0; root < 2; root++ )
      {
        const int a = sbtSkipByRdCost( est, distScale, idx, pos, best, total / 2, trial & 4 ? 1.7e+308 : distScale * double( total / 2 ) + 90000.0, root );
        CHECK( a == 0 || a == 1 || a == 2 || a == 3 || a == 255 );
        if( ( trial & 4 ) && a != 0 ) CHECK( a == 255 );
        if( root ) CHECK( a != 1 && a != 2 ); else CHECK( a != 3 );
      }
    }
  }
}

int main()
{
  for( int w : SIDES )
    for( int h : SIDES )
    {
      test_tiles( w, h );
      test_combine( w, h );
    }
  // the literal corner cases
  CHECK( sbtAllowed( 4, 4, 64 ) == 0 && sbtAllowed( 8, 4, 64 ) == ( 1 << SBT_VER_HALF ) && sbtAllowed( 64, 64, 64 ) == 30 && sbtAllowed( 64, 64, 32 ) == 0 );
  CHECK( numSbtModeRdo( 0 ) == 0 && numSbtModeRdo( 2 ) == 2 && numSbtModeRdo( 30 ) == 4 && numSbtModeRdo( 8 ) == 2 );
  CHECK( targetSbtAllowed( 0, 31 ) == 0 && targetSbtAllowed( 5, 63 ) == 0 );
  CHECK( sbtDistShift( 8 ) == 0 && sbtDistShift( 12 ) == 0 );
  printf( "%d failures\n", failures );
  return failures ? 1 : 0;
}
