// test_lfnst_chain.cpp -- vtm_amd/csrc/lfnst_rules.hpp (the mode rule, the shape rules, the table checks and the expansion of the LFNST residual chain) compiled for the
// host.  Built with -fsanitize=address,undefined and run as its own process (tests/test_lfnst_chain_cpp.py).  Every table lives in a heap array of exactly its length,
// so a read past a table -- through a block index, a prediction index or a count -- aborts under ASan: the mode rule over every shape and mode, the scan and region
// rules as permutations, a full expansion of a mixed table checked field by field, then every rejection, one defect per table, each leaving both outputs untouched.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "../vtm_amd/csrc/lfnst_rules.hpp"

static int failures = 0;
#define CHECK( cond )                                                          \
  do {                                                                         \
    if( !( cond ) ) { failures++; printf( "%s:%d: %s\n", __FILE__, __LINE__, #cond ); } \
  } while( 0 )

struct Tables
{
  std::vector<vtmhip_intra_block>        blocks;
  std::vector<vtmhip_intra_job>          intra;
  std::vector<vtmhip_mip_job>            mip;
  std::vector<vtmhip_intra_tu_job>       tu;
  std::vector<vtmhip_intra_lfnst_tu_job> lf;
};

static vtmhip_intra_block blockOf( int w, int h, int bd, int m, int64_t orgOff )
{
  vtmhip_intra_block b;
  memset( &b, 0, sizeof( b ) );
  b.refOff = 1000 + orgOff; b.orgOff = orgOff; b.orgStride = 97; b.width = ( int16_t ) w; b.height = ( int16_t ) h; b.bitDepth = ( uint8_t ) bd; b.multiRefIdx = ( uint8_t ) m;
  return b;
}

// 8x8, 16x4 on line 1, 64x16, 4x16, 16x16, 4x4; regular jobs on all, MIP jobs on the 8x8, 64x16 and 16x16 blocks; plain and LFNST candidates name the same predictions
static Tables baseTables()
{
  Tables T;
  T.blocks = { blockOf( 8, 8, 10, 0, 101 ), blockOf( 16, 4, 8, 1, 2001 ), blockOf( 64, 16, 12, 0, 4001 ), blockOf( 4, 16, 10, 2, 9001 ), blockOf( 16, 16, 8, 0, 9501 ),
               blockOf( 4, 4, 12, 0, 9901 ) };
  const int modes[][2] = { { 0, 0 }, { 0, 50 }, { 1, 3 }, { 1, 18 }, { 2, 34 }, { 3, 64 }, { 3, 2 }, { 4, 1 }, { 4, 66 }, { 5, 20 } };   // (block, mode)
  int64_t off = 3;
  for( const auto &m : modes )
  {
    vtmhip_intra_job j;
    memset( &j, 0, sizeof( j ) );
    j.predOff = off; j.block = m[0]; j.mode = ( uint8_t ) m[1];
    off += T.blocks[m[0]].width * T.blocks[m[0]].height + 5;
    T.intra.push_back( j );
  }
  const int mips[][3] = { { 0, 7, 1 }, { 2, 5, 0 }, { 4, 0, 1 } };   // (block, mode, transposed)
  for( const auto &m : mips )
  {
    vtmhip_mip_job j;
    memset( &j, 0, sizeof( j ) );
    j.predOff = off; j.block = m[0]; j.mode = ( uint8_t ) m[1]; j.transposed = ( uint8_t ) m[2];
    off += T.blocks[m[0]].width * T.blocks[m[0]].height + 5;
    T.mip.push_back( j );
  }
  int64_t out = 7;
  const int nPred = ( int ) ( T.intra.size() + T.mip.size() );
  for( int p = 0; p < nPred; p += 2 )
  {
    vtmhip_intra_tu_job t;
    memset( &t, 0, sizeof( t ) );
    t.outOff = out; t.pred = p; t.qpPer = 4; t.qpRem = ( int16_t ) ( p % 6 ); t.typeHor = VTMHIP_DCT2; t.typeVer = VTMHIP_DCT2; t.isIRAP = ( uint8_t ) ( p & 1 );
    out += 4096 + 5;
    T.tu.push_back( t );
  }
  for( int p = nPred - 1; p >= 0; p-- )   // the LFNST table runs backwards through the predictions: a shuffled table
  {
    if( p == 10 ) continue;               // MIP on the 8x8 block: not admissible
    for( int idx = 1; idx <= ( p % 3 ? 1 : 2 ); idx++ )
    {
      vtmhip_intra_lfnst_tu_job t;
      memset( &t, 0, sizeof( t ) );
      t.outOff = out; t.pred = p; t.qpPer = ( int16_t ) ( 3 + idx ); t.qpRem = ( int16_t ) ( ( p + idx ) % 6 ); t.lfnstIdx = ( uint8_t ) ( p % 3 ? 1 + ( p & 1 ) : idx );
      t.isIRAP = ( uint8_t ) ( ( p + idx ) & 1 );
      out += 4096 + 5;
      T.lf.push_back( t );
    }
  }
  return T;
}

// every table copied into a heap array of exactly its length (empty: nullptr)
template<class T> static T *exact( const std::vector<T> &v )
{
  if( v.empty() ) return nullptr;
  T *p = ( T * ) malloc( v.size() * sizeof( T ) );
  memcpy( p, v.data(), v.size() * sizeof( T ) );
  return p;
}

struct Run
{
  bool ok;
  std::vector<vtmhip_tu_job>          tu;
  std::vector<vtmhip_lfnst_chain_job> lf;
  IntraChainPlan plan;
  LfnstPlan      lplan;
  bool           untouched;
};

static Run run( const Tables &T )
{
  vtmhip_intra_block *b = exact( T.blocks ); vtmhip_intra_job *ij = exact( T.intra ); vtmhip_mip_job *mj = exact( T.mip ); vtmhip_intra_tu_job *tj = exact( T.tu );
  vtmhip_intra_lfnst_tu_job *lj = exact( T.lf );
  Run r;
  r.tu.resize( T.tu.size() ); r.lf.resize( T.lf.size() );
  vtmhip_tu_job          *ot = ( vtmhip_tu_job * ) malloc( T.tu.size() * sizeof( vtmhip_tu_job ) + 1 );
  vtmhip_lfnst_chain_job *ol = ( vtmhip_lfnst_chain_job * ) malloc( T.lf.size() * sizeof( vtmhip_lfnst_chain_job ) + 1 );
  memset( ot, 0xa5, T.tu.size() * sizeof( vtmhip_tu_job ) );
  memset( ol, 0xa5, T.lf.size() * sizeof( vtmhip_lfnst_chain_job ) );
  r.ok = lfnstLevelMakeJobs( b, ( int ) T.blocks.size(), ij, ( int ) T.intra.size(), mj, ( int ) T.mip.size(), tj, ( int ) T.tu.size(), lj, ( int ) T.lf.size(), ot, ol, r.plan,
                             r.lplan );
  r.untouched = true;
  for( size_t i = 0; i < T.tu.size() * sizeof( vtmhip_tu_job ); i++ ) r.untouched = r.untouched && ( ( unsigned char * ) ot )[i] == 0xa5;
  for( size_t i = 0; i < T.lf.size() * sizeof( vtmhip_lfnst_chain_job ); i++ ) r.untouched = r.untouched && ( ( unsigned char * ) ol )[i] == 0xa5;
  if( !T.tu.empty() ) memcpy( r.tu.data(), ot, T.tu.size() * sizeof( vtmhip_tu_job ) );
  if( !T.lf.empty() ) memcpy( r.lf.data(), ol, T.lf.size() * sizeof( vtmhip_lfnst_chain_job ) );
  free( b ); free( ij ); free( mj ); free( tj ); free( lj ); free( ot ); free( ol );
  return r;
}

// the mode rule written a second way: the table of H.266 8.7.4.1 as an array over the wide-angle modes -14 .. 80
static void modeRule()
{
  int lut[95];
  for( int m = -14; m <= 80; m++ ) lut[m + 14] = m < 0 ? 1 : m <= 1 ? 0 : m <= 12 ? 1 : m <= 23 ? 2 : m <= 44 ? 3 : m <= 55 ? 2 : 1;
  const int sides[5] = { 4, 8, 16, 32, 64 }, shift[6] = { 0, 6, 10, 12, 14, 15 };
  int cases = 0, wideLo = 0, wideHi = 0;
  for( int w : sides )
    for( int h : sides )
      for( int mode = 0; mode < 67; mode++ )
      {
        const int d = abs( intraLog2( w ) - intraLog2( h ) );
        int wide = mode;
        if( mode > 1 && w > h && mode < 2 + shift[d] ) wide = mode + 65;
        if( mode > 1 && h > w && mode > 66 - shift[d] ) wide = mode - 67;
        if( wide < wideLo ) wideLo = wide;
        if( wide > wideHi ) wideHi = wide;
        int s, t;
        lfnstModeOf( w, h, mode, false, s, t );
        CHECK( lfnstWideAngle( w, h, mode ) == wide );
        CHECK( s == lut[wide + 14] );
        CHECK( t == ( wide > 66 || ( wide > 34 && wide <= 66 ) ? 1 : 0 ) );   // past the diagonal, the flat block's modes above 66 included; the tall block's below 0 not
        lfnstModeOf( w, h, mode, true, s, t );
        CHECK( s == 0 && t == 0 );
        cases++;
      }
  CHECK( cases == 25 * 67 && wideLo == -14 && wideHi == 80 );
}

static void shapeRules()
{
  const int sides[5] = { 4, 8, 16, 32, 64 };
  for( int w : sides )
    for( int h : sides )
    {
      const bool sb8 = w >= 8 && h >= 8;
      const int  keep = lfnstKeep( w, h ), trSize = lfnstTrSize( w, h ), zo = lfnstZeroOut( w, h );
      CHECK( keep == ( ( w == 4 || h == 4 ) ? 4 : 8 ) && trSize == ( sb8 ? 48 : 16 ) && zo == ( ( w == h && w <= 8 ) ? 8 : 16 ) );
      CHECK( lfnstShapeOk( w, h, false ) && lfnstShapeOk( w, h, true ) == ( w >= 16 && h >= 16 ) );
      // the scan positions are distinct, inside the region, and the first 16 inside the top-left 4x4; the region rule is a permutation of the same set
      std::vector<int> seenScan( ( size_t ) w * h, 0 ), seenReg( ( size_t ) w * h, 0 );
      for( int k = 0; k < trSize; k++ )
      {
        const int p = lfnstScanPos( k, w, sb8 ), x = p % w, y = p / w;
        CHECK( p >= 0 && p < w * h && x < keep && y < keep && !( x >= 4 && y >= 4 ) && !seenScan[p] );
        if( k < 16 ) CHECK( x < 4 && y < 4 && lfnstScanPos( k, 4, false ) == x + 4 * y );
        seenScan[p] = 1;
      }
      for( int tr = 0; tr < 2; tr++ )
      {
        std::fill( seenReg.begin(), seenReg.end(), 0 );
        for( int v = 0; v < trSize; v++ )
        {
          int x, y, xt, yt;
          lfnstRegionXY( v, sb8, tr != 0, x, y );
          lfnstRegionXY( v, sb8, tr == 0, xt, yt );
          CHECK( x == yt && y == xt && x >= 0 && y >= 0 && x < keep && y < keep && !seenReg[y * w + x] );
          seenReg[y * w + x] = 1;
        }
        CHECK( seenReg == seenScan );
      }
      CHECK( lfnstJobInts( w, h ) * ( 256 / lfnstLanes( w * h ) ) * 4 <= 64 * 1024 );   // the LDS of a workgroup of such jobs
    }
  CHECK( lfnstLanes( 16 ) == 16 && lfnstLanes( 256 ) == 16 && lfnstLanes( 512 ) == 64 && lfnstLanes( 4096 ) == 64 );
}

int main()
{
  modeRule();
  shapeRules();

  // the full expansion
  const Tables T = baseTables();
  const Run    r = run( T );
  CHECK( r.ok && !r.untouched );
  CHECK( r.lplan.maxArea == 64 * 16 && lfnstLanes( r.lplan.maxArea ) == 64 && r.lplan.jobInts == lfnstJobInts( 64, 16 ) );
  CHECK( r.plan.tu.maxWidth == 64 && r.plan.tu.maxHeight == 16 && r.plan.tu.uniform == 0 );
  const int nIntra = ( int ) T.intra.size();
  for( size_t i = 0; i < T.lf.size(); i++ )
  {
    const vtmhip_intra_lfnst_tu_job &t = T.lf[i];
    const bool    isMip   = t.pred >= nIntra;
    const int     blk     = isMip ? T.mip[t.pred - nIntra].block : T.intra[t.pred].block;
    const int64_t predOff = isMip ? T.mip[t.pred - nIntra].predOff : T.intra[t.pred].predOff;
    const vtmhip_intra_block     &b = T.blocks[blk];
    const vtmhip_lfnst_chain_job &o = r.lf[i];
    int s, tr;
    lfnstModeOf( b.width, b.height, isMip ? 0 : T.intra[t.pred].mode, isMip, s, tr );
    CHECK( o.resiOff == predOff && o.outOff == t.outOff && o.resiStride == b.width && o.width == b.width && o.height == b.height );
    CHECK( o.qpPer == t.qpPer && o.qpRem == t.qpRem && o.bitDepth == b.bitDepth && o.isIRAP == t.isIRAP && o.setIdx == s && o.index == t.lfnstIdx - 1 && o.transpose == tr );
    for( int k = 0; k < 7; k++ ) CHECK( o.pad[k] == 0 );
    CHECK( lfnstChainJobOk( o ) );
  }
  for( size_t i = 0; i < T.tu.size(); i++ ) CHECK( r.tu[i].outOff == T.tu[i].outOff && r.tu[i].typeHor == VTMHIP_DCT2 && r.tu[i].pad == 0 );
  // 16x4 mode 3 is the wide angle 68 (set 1, transposed), 4x16 mode 64 the wide angle -3 (set 1, not transposed), MIP is planar
  {
    int s, t;
    lfnstModeOf( 16, 4, 3, false, s, t );  CHECK( s == 1 && t == 1 );
    lfnstModeOf( 4, 16, 64, false, s, t ); CHECK( s == 1 && t == 0 );
    lfnstModeOf( 16, 16, 66, true, s, t ); CHECK( s == 0 && t == 0 );
  }
  // empty tables
  {
    Tables E = T; E.lf.clear();
    const Run e = run( E );
    CHECK( e.ok && e.lplan.maxArea == 0 && e.lplan.jobInts == 0 );
    E = T; E.tu.clear();
    const Run f = run( E );
    CHECK( f.ok && f.plan.tu.maxWidth == 0 && f.lplan.maxArea == 64 * 16 );
    const Run g = run( Tables() );
    CHECK( g.ok );
  }

  // one defect per table
  typedef std::function<void( Tables & )> Defect;
  const std::vector<Defect> defects = {
    []( Tables &t ) { t.lf[1].lfnstIdx = 0; }, []( Tables &t ) { t.lf[1].lfnstIdx = 3; },
    []( Tables &t ) { t.lf[0].pred = 10; },                      // MIP on the 8x8 block
    []( Tables &t ) { t.lf[2].pred = 13; }, []( Tables &t ) { t.lf[2].pred = -1; },
    []( Tables &t ) { t.lf[3].qpRem = 6; }, []( Tables &t ) { t.lf[3].qpRem = -1; }, []( Tables &t ) { t.lf[3].qpPer = -1; },
    []( Tables &t ) { t.lf[4].reserved[0] = 1; }, []( Tables &t ) { t.lf[4].reserved[1] = 1; }, []( Tables &t ) { t.lf[4].pad = 1; },
    []( Tables &t ) { t.blocks[2].width = 12; }, []( Tables &t ) { t.blocks[0].bitDepth = 13; }, []( Tables &t ) { t.intra[1].mode = 67; },
    []( Tables &t ) { t.tu[0].typeHor = 4; }, []( Tables &t ) { t.tu[1].reserved = 1; },
  };
  int rejected = 0;
  for( const Defect &d : defects )
  {
    Tables B = baseTables();
    d( B );
    const Run q = run( B );
    CHECK( !q.ok && q.untouched );
    rejected += !q.ok && q.untouched;
  }
  // the chain's own table
  {
    std::vector<vtmhip_lfnst_chain_job> jobs = r.lf;
    LfnstPlan p;
    vtmhip_lfnst_chain_job *e = exact( jobs );
    CHECK( lfnstChainScan( e, ( int ) jobs.size(), p ) && p.maxArea == 64 * 16 );
    free( e );
    const std::vector<std::function<void( vtmhip_lfnst_chain_job & )>> bad = {
      []( vtmhip_lfnst_chain_job &j ) { j.width = 12; }, []( vtmhip_lfnst_chain_job &j ) { j.height = 128; }, []( vtmhip_lfnst_chain_job &j ) { j.resiStride = j.width - 1; },
      []( vtmhip_lfnst_chain_job &j ) { j.bitDepth = 7; }, []( vtmhip_lfnst_chain_job &j ) { j.qpRem = 6; }, []( vtmhip_lfnst_chain_job &j ) { j.qpPer = -1; },
      []( vtmhip_lfnst_chain_job &j ) { j.setIdx = 4; }, []( vtmhip_lfnst_chain_job &j ) { j.index = 2; }, []( vtmhip_lfnst_chain_job &j ) { j.transpose = 2; },
      []( vtmhip_lfnst_chain_job &j ) { j.pad[3] = 1; },
    };
    for( const auto &f : bad )
    {
      std::vector<vtmhip_lfnst_chain_job> c = jobs;
      f( c[c.size() - 1] );
      vtmhip_lfnst_chain_job *x = exact( c );
      const bool ok = lfnstChainScan( x, ( int ) c.size(), p );
      CHECK( !ok );
      rejected += !ok;
      free( x );
    }
  }
  printf( "%d of %d malformed tables rejected\n", rejected, ( int ) defects.size() + 10 );
  printf( "%d failures\n", failures );
  return failures != 0;
}
