// test_mmvd.cpp -- the MMVD rules of vtm_amd/csrc/mmvd_rules.hpp (HIP-free) as a stand-alone program under AddressSanitizer and UBSan (tests/test_mmvd_cpp.py builds
// and runs it).  Randomised jobs go through the table predicate and the derivation; every job, record array and vector array sits in a heap array of exactly its
// length, so a read or write past one is a report, and the arithmetic (shifts, products of POC differences, the scaled offsets) runs under UBSan.  What the derivation
// leaves is checked for what can be said without a second implementation: the tested set is the loop's, stored vectors stay inside the storage range and move from
// the base by the step on one component only, the carrier list moves by exactly the step and the other list by no more and with the sign the POC sides give, 8x4 / 4x8
// never stay bi, BDOF kinds appear exactly where the base allows them and only up to step 2, prediction vectors lie inside clipMv's limits and equal the stored ones
// when those do.  The predicate rejects each malformed field.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>

#include "../vtm_amd/csrc/mmvd_rules.hpp"

static int g_failures = 0;
#define EXPECT( cond ) do { if( !( cond ) ) { g_failures++; if( g_failures < 20 ) printf( "FAIL %s:%d %s\n", __FILE__, __LINE__, #cond ); } } while( 0 )

template<class T> static std::unique_ptr<T[]> heap( size_t n ) { return std::unique_ptr<T[]>( new T[n]() ); }

static const int PIC_W = 416, PIC_H = 240, CTU = 128;

static void random_job( std::mt19937 &rng, vtmhip_mmvd_job &j )
{
  static const int sides[6] = { 4, 8, 16, 32, 64, 128 }, bcw[5] = { -2, 3, 4, 5, 10 };
  j = vtmhip_mmvd_job();
  do { j.width = ( int16_t ) sides[rng() % 6]; j.height = ( int16_t ) sides[rng() % 6]; } while( j.width == 4 && j.height == 4 );
  j.orgStride = j.width + ( int ) ( rng() % 3 ) * 8;
  j.posX = ( int ) ( rng() % ( PIC_W / 4 ) ) * 4; j.posY = ( int ) ( rng() % ( PIC_H / 4 ) ) * 4;
  j.bitDepth = ( uint8_t ) ( 8 + rng() % 5 ); j.numBase = ( uint8_t ) ( 1 + rng() % 2 ); j.numSteps = ( uint8_t ) ( 1 + rng() % 8 );
  j.disFracMmvd = ( uint8_t ) ( rng() % 2 ); j.bdofAllowed = ( uint8_t ) ( rng() % 4 != 0 );
  for( int b = 0; b < 2; b++ )
  {
    vtmhip_mmvd_base &s = j.base[b];
    const int kind = ( int ) ( rng() % 4 );   // 0: list 0, 1: list 1, 2 / 3: bi
    s.refIdx[0] = ( int8_t ) ( kind == 1 ? -1 : rng() % 3 ); s.refIdx[1] = ( int8_t ) ( kind == 0 ? -1 : rng() % 3 );
    for( int l = 0; l < 2; l++ )
    {
      const bool edge = rng() % 8 == 0;
      s.mv[l][0] = edge ? ( rng() % 2 ? ( 1 << 17 ) - 1 - ( int ) ( rng() % 200 ) : -( 1 << 17 ) + ( int ) ( rng() % 200 ) ) : ( int ) ( rng() % 4096 ) - 2048;
      s.mv[l][1] = edge ? ( rng() % 2 ? ( 1 << 17 ) - 1 - ( int ) ( rng() % 200 ) : -( 1 << 17 ) + ( int ) ( rng() % 200 ) ) : ( int ) ( rng() % 4096 ) - 2048;
      s.refStride[l] = j.width + 64; s.refOff[l] = 0;
      int d = ( int ) ( rng() % 16 ) + 1;
      if( rng() % 16 == 0 ) d += 120 + ( int ) ( rng() % 200 );   // beyond the +-128 clip
      s.pocDiff[l] = rng() % 2 ? d : -d;
      s.longTerm[l] = ( uint8_t ) ( rng() % 6 == 0 );
    }
    if( rng() % 3 == 0 ) s.pocDiff[1] = rng() % 2 ? s.pocDiff[0] : -s.pocDiff[0];   // equal differences / equal distance on opposite sides
    s.useAltHpelIf = ( uint8_t ) ( rng() % 2 );
    s.bcwWeightL1  = ( int8_t ) ( rng() % 2 ? 4 : bcw[rng() % 5] );
  }
}

static int sgn( long long v ) { return v > 0 ? 1 : v < 0 ? -1 : 0; }

static void check_job( const vtmhip_mmvd_job &j, long &cands )
{
  EXPECT( mmvdJobOk( j ) );
  auto rec = heap<vtmhip_mmvd_cand>( VTMHIP_MMVD_NUM_CAND );
  auto pmv = heap<int32_t[2][2]>( VTMHIP_MMVD_NUM_CAND );
  int  numBdof = 0, numTested = 0;
  for( int c = 0; c < VTMHIP_MMVD_NUM_CAND; c++ )
  {
    int mode = -1;
    mmvdDerive( j, PIC_W, PIC_H, CTU, c, rec[c], mode, pmv[c] );
    cands++;
    const vtmhip_mmvd_cand &r = rec[c];
    const int  b = c / 32, step = ( c % 32 ) / 4, pos = c % 4;
    const bool inLoop = c < ( j.numBase > 1 ? 64 : 32 ) && step < j.numSteps;
    EXPECT( ( r.kind != VTMHIP_MMVD_NOT_TESTED ) == inLoop );
    if( !inLoop )
    {
      EXPECT( r.interDir == 0 && r.refIdx[0] == -1 && r.refIdx[1] == -1 && r.mv[0][0] == 0 && r.mv[0][1] == 0 && r.mv[1][0] == 0 && r.mv[1][1] == 0 && r.bcwWeightL1 == 0 );
      EXPECT( pmv[c][0][0] == 0 && pmv[c][0][1] == 0 && pmv[c][1][0] == 0 && pmv[c][1][1] == 0 );
      continue;
    }
    numTested++;
    numBdof += r.kind == VTMHIP_MMVD_BDOF;
    const vtmhip_mmvd_base &s = j.base[b];
    const bool baseBi = s.refIdx[0] >= 0 && s.refIdx[1] >= 0, small = j.width + j.height == 12;
    const int  offset = mmvdOffset( step, j.disFracMmvd ), comp = pos >> 1, dir = ( pos & 1 ) ? -1 : 1;
    EXPECT( offset == ( 4 << step ) * ( j.disFracMmvd ? 4 : 1 ) );
    EXPECT( r.interDir == ( baseBi ? ( small ? 1 : 3 ) : s.refIdx[0] >= 0 ? 1 : 2 ) );
    EXPECT( r.bcwWeightL1 == ( r.interDir == 3 ? s.bcwWeightL1 : 4 ) && r.useAltHpelIf == s.useAltHpelIf );
    const int carrier = !baseBi ? ( s.refIdx[0] >= 0 ? 0 : 1 ) : ( mmvdAbs( s.pocDiff[1] ) > mmvdAbs( s.pocDiff[0] ) ? 1 : 0 );
    for( int l = 0; l < 2; l++ )
    {
      const bool used = r.interDir >> l & 1;
      EXPECT( r.refIdx[l] == ( used ? s.refIdx[l] : -1 ) );
      if( !used ) { EXPECT( r.mv[l][0] == 0 && r.mv[l][1] == 0 && pmv[c][l][0] == 0 && pmv[c][l][1] == 0 ); continue; }
      EXPECT( r.mv[l][0] >= -( 1 << 17 ) && r.mv[l][0] < ( 1 << 17 ) && r.mv[l][1] >= -( 1 << 17 ) && r.mv[l][1] < ( 1 << 17 ) );
      EXPECT( r.mv[l][1 - comp] == s.mv[l][1 - comp] );   // the other component stays (base vectors are inside the storage range)
      const int moved = r.mv[l][comp] - s.mv[l][comp], want = mmvdStorageClip( s.mv[l][comp] + dir * offset ) - s.mv[l][comp];
      if( l == carrier ) EXPECT( moved == want );
      else
      {
        // the other list of a bi base: no further than the step, towards the side the POC differences give (nothing where the scaled offset rounds to 0).  The
        // factor is at most 256 of 256 in magnitude, but 258 where both differences lie beyond the clip (-128 over 127: ( 128 * 129 + 32 ) >> 6)
        EXPECT( mmvdAbs( moved ) <= offset + offset / 64 );
        const int side = sgn( ( long long ) s.pocDiff[0] * s.pocDiff[1] );
        if( moved != 0 && mmvdStorageClip( s.mv[l][comp] + moved ) == s.mv[l][comp] + moved ) EXPECT( sgn( moved ) == dir * side );
        if( s.pocDiff[0] == s.pocDiff[1] ) EXPECT( moved == want );
      }
    }
    if( r.kind == VTMHIP_MMVD_BDOF )
      EXPECT( j.bdofAllowed && r.interDir == 3 && step <= 2 && j.width >= 8 && j.height >= 8 && j.width * j.height >= 128 && r.bcwWeightL1 == 4 && !s.longTerm[0] &&
              !s.longTerm[1] && s.pocDiff[0] == -s.pocDiff[1] && mmvdBaseBdof( j, b ) );
    else EXPECT( !( mmvdBaseBdof( j, b ) && step <= 2 ) );
    EXPECT( mode == MMVD_PRED_L0 || mode == MMVD_PRED_L1 || mode == MMVD_PRED_BI );
    if( r.interDir != 3 ) EXPECT( mode == ( r.interDir == 2 ? MMVD_PRED_L1 : MMVD_PRED_L0 ) );
    else EXPECT( ( mode == MMVD_PRED_L0 ) == ( s.pocDiff[0] == s.pocDiff[1] && r.mv[0][0] == r.mv[1][0] && r.mv[0][1] == r.mv[1][1] ) );
    for( int l = 0; l < 2; l++ )
    {
      if( !( mode == MMVD_PRED_BI || mode == l ) ) { EXPECT( pmv[c][l][0] == 0 && pmv[c][l][1] == 0 ); continue; }
      const int lim[2][2] = { { mmvdClipMin( CTU, j.posX ), mmvdClipMax( PIC_W, j.posX ) }, { mmvdClipMin( CTU, j.posY ), mmvdClipMax( PIC_H, j.posY ) } };
      for( int k = 0; k < 2; k++ )
      {
        EXPECT( pmv[c][l][k] >= lim[k][0] && pmv[c][l][k] <= lim[k][1] );
        if( r.mv[l][k] >= lim[k][0] && r.mv[l][k] <= lim[k][1] ) EXPECT( pmv[c][l][k] == r.mv[l][k] );
      }
    }
  }
  EXPECT( numTested == mmvdNumTested( j ) && numBdof == mmvdNumBdof( j ) && numBdof <= MMVD_BDOF_MAX );
}

static void check_predicate()
{
  std::mt19937 rng( 11 );
  for( int it = 0; it < 200; it++ )
  {
    auto jp = heap<vtmhip_mmvd_job>( 1 );
    vtmhip_mmvd_job &j = jp[0];
    random_job( rng, j );
    j.numBase = 2;
    EXPECT( mmvdJobOk( j ) );
    vtmhip_mmvd_job m;
#define REJECT( change ) do { m = j; change; EXPECT( !mmvdJobOk( m ) ); } while( 0 )
    REJECT( m.width = 2 ); REJECT( m.width = 12 ); REJECT( m.width = 256 ); REJECT( m.height = 0 ); REJECT( m.height = 24 ); REJECT( m.height = -8 );
    REJECT( m.width = 4; m.height = 4 );
    REJECT( m.numBase = 0 ); REJECT( m.numBase = 3 ); REJECT( m.numSteps = 0 ); REJECT( m.numSteps = 9 );
    REJECT( m.bitDepth = 7 ); REJECT( m.bitDepth = 13 ); REJECT( m.orgStride = m.width - 1 );
    for( int b = 0; b < 2; b++ )
    {
      REJECT( m.base[b].refIdx[0] = m.base[b].refIdx[1] = -1 );
      REJECT( m.base[b].bcwWeightL1 = 0 ); REJECT( m.base[b].bcwWeightL1 = 6 ); REJECT( m.base[b].bcwWeightL1 = -1 );
      for( int l = 0; l < 2; l++ )
        if( j.base[b].refIdx[l] >= 0 ) REJECT( m.base[b].refStride[l] = m.width - 1 );
    }
#undef REJECT
    // the second base is not looked at when the loop does not reach it
    m = j; m.numBase = 1; m.base[1].refIdx[0] = m.base[1].refIdx[1] = -1; m.base[1].bcwWeightL1 = 0;
    EXPECT( mmvdJobOk( m ) );
  }
}

static void check_scale()
{
  EXPECT( mmvdDistScaleFactor( 3, 3 ) == 4096 && mmvdDistScaleFactor( -7, -7 ) == 4096 );
  // a mirrored distance mirrors the offset: the factor is -256 of 256 while d * ( ( 0x4000 + d / 2 ) / d ) > 16352, which d <= 63 guarantees (the product is at
  // least 0x4000 + d / 2 - ( d - 1 )); beyond that the table's rounding may give -255 (d = 83 does)
  for( int d = 1; d <= 63; d++ )
    for( int v = -8192; v <= 8192; v += 4 )
      EXPECT( mmvdDistScaleFactor( -d, d ) == -256 && mmvdScaleMv( mmvdDistScaleFactor( -d, d ), v ) == -v );
  EXPECT( mmvdDistScaleFactor( -83, 83 ) == -255 );
  EXPECT( mmvdDistScaleFactor( 1000, -1000 ) == mmvdDistScaleFactor( 127, -128 ) );   // the clip of the POC differences
  EXPECT( mmvdScaleMv( 4095, ( 1 << 17 ) - 1 ) <= ( 1 << 17 ) - 1 && mmvdScaleMv( -4096, -( 1 << 17 ) ) == ( 1 << 17 ) - 1 );
}

int main()
{
  std::mt19937 rng( 2026 );
  long         jobs = 0, cands = 0;
  for( int it = 0; it < 20000; it++ )
  {
    auto jp = heap<vtmhip_mmvd_job>( 1 );
    random_job( rng, jp[0] );
    check_job( jp[0], cands );
    jobs++;
  }
  check_predicate();
  check_scale();
  printf( "mmvd rules: %ld jobs, %ld candidates, %d failures\n", jobs, cands, g_failures );
  return g_failures ? 1 : 0;
}
