// test_intra_chain.cpp -- vtm_amd/csrc/intra_chain_rules.hpp (the table checks and the TU-job expansion of vtmhip_intra_chain_batch_dev) compiled for the host.  Built
// with -fsanitize=address,undefined and run as its own process (tests/test_intra_chain_cpp.py).  Every table lives in a heap array of exactly its length, so a read
// past a table -- through a block index, a prediction index or a count -- aborts under ASan: a full expansion of a mixed table checked field by field, then every
// rejection, one defect per table, each leaving `out` untouched.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "../vtm_amd/csrc/intra_chain_rules.hpp"

static int failures = 0;
#define CHECK( cond )                                                          \
  do {                                                                         \
    if( !( cond ) ) { failures++; printf( "%s:%d: %s\n", __FILE__, __LINE__, #cond ); } \
  } while( 0 )

struct Tables
{
  std::vector<vtmhip_intra_block>  blocks;
  std::vector<vtmhip_intra_job>    intra;
  std::vector<vtmhip_mip_job>      mip;
  std::vector<vtmhip_intra_tu_job> tu;
};

static vtmhip_intra_block blockOf( int w, int h, int bd, int m, int64_t orgOff )
{
  vtmhip_intra_block b;
  memset( &b, 0, sizeof( b ) );
  b.refOff = 1000 + orgOff; b.orgOff = orgOff; b.orgStride = 97; b.width = ( int16_t ) w; b.height = ( int16_t ) h; b.bitDepth = ( uint8_t ) bd; b.multiRefIdx = ( uint8_t ) m;
  return b;
}

static vtmhip_intra_tu_job tuOf( int pred, int th, int tv, int qpPer, int qpRem, int irap, int64_t outOff )
{
  vtmhip_intra_tu_job t;
  memset( &t, 0, sizeof( t ) );
  t.outOff = outOff; t.pred = pred; t.qpPer = ( int16_t ) qpPer; t.qpRem = ( int16_t ) qpRem; t.typeHor = ( uint8_t ) th; t.typeVer = ( uint8_t ) tv; t.isIRAP = ( uint8_t ) irap;
  return t;
}

// 8x8 on line 0, 16x4 on line 1, 64x16 on line 0, 32x32 on line 2; regular jobs on all, MIP jobs on the line-0 blocks; 1 .. 4 candidates per prediction
static Tables baseTables()
{
  Tables T;
  T.blocks = { blockOf( 8, 8, 10, 0, 101 ), blockOf( 16, 4, 8, 1, 2001 ), blockOf( 64, 16, 12, 0, 4001 ), blockOf( 32, 32, 10, 2, 9001 ) };
  const int modes[][2] = { { 0, 0 }, { 0, 50 }, { 1, 1 }, { 1, 18 }, { 2, 34 }, { 3, 66 }, { 3, 2 } };   // (block, mode)
  int64_t off = 3;
  for( const auto &m : modes )
  {
    vtmhip_intra_job j;
    memset( &j, 0, sizeof( j ) );
    j.predOff = off; j.block = m[0]; j.mode = ( uint8_t ) m[1];
    off += T.blocks[m[0]].width * T.blocks[m[0]].height + 5;
    T.intra.push_back( j );
  }
  const int mips[][3] = { { 0, 7, 1 }, { 2, 5, 0 }, { 0, 0, 0 } };   // (block, mode, transposed)
  for( const auto &m : mips )
  {
    vtmhip_mip_job j;
    memset( &j, 0, sizeof( j ) );
    j.predOff = off; j.block = m[0]; j.mode = ( uint8_t ) m[1]; j.transposed = ( uint8_t ) m[2];
    off += T.blocks[m[0]].width * T.blocks[m[0]].height + 5;
    T.mip.push_back( j );
  }
  const int cands[4][2] = { { VTMHIP_DCT2, VTMHIP_DCT2 }, { VTMHIP_DST7, VTMHIP_DST7 }, { VTMHIP_DCT8, VTMHIP_DST7 }, { VTMHIP_TRSKIP, VTMHIP_TRSKIP } };
  int64_t out = 7;
  for( int p = 0; p < ( int ) ( T.intra.size() + T.mip.size() ); p++ )
  {
    const int blk = p < ( int ) T.intra.size() ? T.intra[p].block : T.mip[p - T.intra.size()].block;
    const int n   = T.blocks[blk].width > 32 ? 1 : 1 + p % 4;
    for( int k = 0; k < n; k++ )
    {
      T.tu.push_back( tuOf( p, cands[k][0], cands[k][1], 3 + p, ( p + k ) % 6, k & 1, out ) );
      out += T.blocks[blk].width * T.blocks[blk].height + 5;
    }
  }
  return T;
}

// the tables copied into heap arrays of exactly their length (an empty table: a null pointer)
template<typename T> static T *exact( const std::vector<T> &v )
{
  if( v.empty() ) return nullptr;
  T *p = ( T * ) malloc( v.size() * sizeof( T ) );
  memcpy( p, v.data(), v.size() * sizeof( T ) );
  return p;
}

static bool run( const Tables &T, std::vector<vtmhip_tu_job> &out, IntraChainPlan &plan )
{
  vtmhip_intra_block  *b = exact( T.blocks );
  vtmhip_intra_job    *i = exact( T.intra );
  vtmhip_mip_job      *m = exact( T.mip );
  vtmhip_intra_tu_job *t = exact( T.tu );
  vtmhip_tu_job       *o = ( vtmhip_tu_job * ) malloc( T.tu.size() * sizeof( vtmhip_tu_job ) + 1 );
  memset( o, 0xa5, T.tu.size() * sizeof( vtmhip_tu_job ) );
  const bool ok = intraChainMakeTuJobs( b, ( int ) T.blocks.size(), i, ( int ) T.intra.size(), m, ( int ) T.mip.size(), t, ( int ) T.tu.size(), o, plan );
  out.assign( o, o + T.tu.size() );
  free( b ); free( i ); free( m ); free( t ); free( o );
  return ok;
}

static bool untouched( const std::vector<vtmhip_tu_job> &out )
{
  const unsigned char *p = ( const unsigned char * ) out.data();
  for( size_t k = 0; k < out.size() * sizeof( vtmhip_tu_job ); k++ )
    if( p[k] != 0xa5 ) return false;
  return true;
}

static void test_expansion()
{
  const Tables T = baseTables();
  std::vector<vtmhip_tu_job> out;
  IntraChainPlan plan;
  CHECK( run( T, out, plan ) );
  CHECK( plan.tu.maxWidth == 64 && plan.tu.maxHeight == 32 && plan.tu.maxArea == 1024 && plan.maxBlockArea == 1024 && plan.tu.uniform == 0 );
  int perPred[10] = {};
  for( size_t k = 0; k < T.tu.size(); k++ )
  {
    const vtmhip_intra_tu_job &t = T.tu[k];
    const bool regular = t.pred < ( int ) T.intra.size();
    const int  blk = regular ? T.intra[t.pred].block : T.mip[t.pred - T.intra.size()].block;
    const int64_t predOff = regular ? T.intra[t.pred].predOff : T.mip[t.pred - T.intra.size()].predOff;
    const vtmhip_intra_block &b = T.blocks[blk];
    const vtmhip_tu_job &o = out[k];
    CHECK( o.resiOff == predOff && o.outOff == t.outOff && o.resiStride == b.width && o.width == b.width && o.height == b.height );
    CHECK( o.qpPer == t.qpPer && o.qpRem == t.qpRem && o.typeHor == t.typeHor && o.typeVer == t.typeVer && o.bitDepth == b.bitDepth && o.isIRAP == t.isIRAP );
    CHECK( o.pad == 0 && o.chromaAdj == 0 );
    perPred[t.pred]++;
  }
  for( int p = 0; p < 10; p++ ) CHECK( perPred[p] >= 1 && perPred[p] <= 4 );

  // one size and real transforms: uniform; one transform-skip job more: not
  Tables U;
  U.blocks = { blockOf( 8, 4, 10, 0, 11 ), blockOf( 8, 4, 8, 2, 301 ) };
  U.intra = { T.intra[0], T.intra[1] };
  U.intra[0].block = 0; U.intra[1].block = 1; U.intra[1].mode = 66;
  U.tu = { tuOf( 0, VTMHIP_DCT2, VTMHIP_DST7, 4, 0, 0, 1 ), tuOf( 1, VTMHIP_DCT8, VTMHIP_DCT2, 4, 5, 1, 41 ), tuOf( 1, VTMHIP_DCT2, VTMHIP_DCT2, 0, 0, 1, 81 ) };
  CHECK( run( U, out, plan ) && plan.tu.uniform == 1 && plan.tu.maxWidth == 8 && plan.tu.maxHeight == 4 && plan.maxBlockArea == 32 );
  U.tu.push_back( tuOf( 0, VTMHIP_TRSKIP, VTMHIP_TRSKIP, 4, 0, 0, 121 ) );
  CHECK( run( U, out, plan ) && plan.tu.uniform == 0 );
  // the prediction pass alone; no table at all
  U.tu.clear();
  CHECK( run( U, out, plan ) && plan.tu.uniform == 0 && plan.tu.maxWidth == 0 && plan.tu.maxHeight == 0 && plan.maxBlockArea == 32 );
  CHECK( run( Tables(), out, plan ) && plan.maxBlockArea == 0 );
}

static void test_rejections()
{
  typedef std::function<void( Tables & )> Defect;
  // base tables: intra jobs 0 .. 1 on block 0, 2 .. 3 on block 1 (line 1), 4 on block 2 (64 wide), 5 .. 6 on block 3 (line 2); MIP jobs on blocks 0, 2, 0
  const std::vector<Defect> defects = {
    []( Tables &T ) { T.blocks[0].width = 128; },  []( Tables &T ) { T.blocks[1].height = 2; },  []( Tables &T ) { T.blocks[3].width = 12; },
    []( Tables &T ) { T.blocks[2].bitDepth = 7; }, []( Tables &T ) { T.blocks[0].bitDepth = 13; }, []( Tables &T ) { T.blocks[1].multiRefIdx = 3; },
    []( Tables &T ) { T.intra[2].mode = 0; },      []( Tables &T ) { T.intra[0].mode = 67; },      []( Tables &T ) { T.intra[1].block = 4; },
    []( Tables &T ) { T.intra[6].block = -1; },    []( Tables &T ) { T.mip[0].mode = 8; },          []( Tables &T ) { T.mip[1].mode = 6; },
    []( Tables &T ) { T.mip[2].transposed = 2; },  []( Tables &T ) { T.mip[0].block = 1; },         []( Tables &T ) { T.mip[1].block = 4; },
    []( Tables &T ) { T.mip[1].block = 1 << 30; }, []( Tables &T ) { T.tu[1].pred = 10; },          []( Tables &T ) { T.tu[0].pred = -1; },
    []( Tables &T ) { T.tu[3].pred = 1 << 30; },   []( Tables &T ) { T.tu[2].qpRem = 6; },          []( Tables &T ) { T.tu[2].qpRem = -1; },
    []( Tables &T ) { T.tu[4].qpPer = -1; },       []( Tables &T ) { T.tu[0].typeHor = 4; },        []( Tables &T ) { T.tu[0].typeVer = 255; },
    []( Tables &T ) { T.tu[0].typeHor = VTMHIP_TRSKIP; },   []( Tables &T ) { T.tu[0].typeVer = VTMHIP_TRSKIP; },
    []( Tables &T ) { for( auto &t : T.tu ) if( t.pred == 4 ) t.typeHor = VTMHIP_DST7; },   // 64 wide
    []( Tables &T ) { for( auto &t : T.tu ) if( t.pred == 4 ) t.typeHor = VTMHIP_DCT8; },
    []( Tables &T ) { for( auto &t : T.tu ) if( t.pred == 4 ) t.typeHor = t.typeVer = VTMHIP_TRSKIP; },
    []( Tables &T ) { T.blocks[2] = blockOf( 16, 64, 12, 0, 4001 ); for( auto &t : T.tu ) if( t.pred == 4 ) t.typeVer = VTMHIP_DST7; },   // 64 high
    []( Tables &T ) { T.tu[5].reserved = 1; },     []( Tables &T ) { T.tu[5].pad = 1; },            []( Tables &T ) { T.blocks[3].reserved[1] = 1; },
    []( Tables &T ) { T.intra[3].reserved[2] = 1; }, []( Tables &T ) { T.mip[2].reserved[0] = 1; },
  };
  int rejected = 0;
  for( const Defect &d : defects )
  {
    Tables T = baseTables();
    d( T );
    std::vector<vtmhip_tu_job> out;
    IntraChainPlan plan;
    const bool ok = run( T, out, plan );
    CHECK( !ok );
    CHECK( untouched( out ) );
    rejected += !ok;
  }
  // 16 x 64 with DST7 across (16 wide) is fine: the rule is per side
  Tables T = baseTables();
  T.blocks[2] = blockOf( 16, 64, 12, 0, 4001 );
  for( auto &t : T.tu ) if( t.pred == 4 ) t.typeHor = VTMHIP_DST7;
  std::vector<vtmhip_tu_job> out;
  IntraChainPlan plan;
  CHECK( run( T, out, plan ) );
  printf( "%d of %d malformed tables rejected\n", rejected, ( int ) defects.size() );
}

int main()
{
  test_expansion();
  test_rejections();
  printf( "%d failures\n", failures );
  return failures ? 1 : 0;
}
