// test_intra_chroma_chain.cpp -- vtm_amd/csrc/intra_chroma_chain_rules.hpp (the table checks and the job expansion of vtmhip_intra_chroma_chain_batch_dev) compiled
// for the host.  Built with -fsanitize=address,undefined and run as its own process (tests/test_intra_chroma_chain_cpp.py).  Every table lives in a heap array of
// exactly its length, so a read past a table -- through a block index, a prediction index or a count -- aborts under ASan: a full expansion of a mixed table
// checked field by field, then every rejection, one defect per table, each leaving both outputs untouched.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "../vtm_amd/csrc/intra_chroma_chain_rules.hpp"

static int failures = 0;
#define CHECK( cond )                                                          \
  do {                                                                         \
    if( !( cond ) ) { failures++; printf( "%s:%d: %s\n", __FILE__, __LINE__, #cond ); } \
  } while( 0 )

struct Tables
{
  std::vector<vtmhip_intra_chroma_block>     blocks;
  std::vector<vtmhip_intra_chroma_job>       jobs;
  std::vector<vtmhip_intra_chroma_tu_job>    tu;
  std::vector<vtmhip_intra_chroma_joint_job> joint;
};

static vtmhip_intra_chroma_block blockOf( int w, int h, int bd, int above, int left, int ar, int bl, int64_t off )
{
  vtmhip_intra_chroma_block b;
  memset( &b, 0, sizeof( b ) );
  b.cbRefOff = 1000 + off; b.crRefOff = 2000 + off; b.cbOrgOff = off; b.crOrgOff = 50000 + off; b.lumaOff = 4 * off; b.orgStride = 97; b.lumaStride = 140;
  b.width = ( int16_t ) w; b.height = ( int16_t ) h; b.aboveRight = ( int16_t ) ar; b.belowLeft = ( int16_t ) bl; b.bitDepth = ( uint8_t ) bd;
  b.above = ( uint8_t ) above; b.left = ( uint8_t ) left;
  return b;
}

static vtmhip_intra_chroma_tu_job tuOf( int pred, int comp, int th, int qpPer, int qpRem, int irap, int adj, int64_t outOff )
{
  vtmhip_intra_chroma_tu_job t;
  memset( &t, 0, sizeof( t ) );
  t.outOff = outOff; t.pred = pred; t.qpPer = ( int16_t ) qpPer; t.qpRem = ( int16_t ) qpRem; t.component = ( uint8_t ) comp; t.typeHor = ( uint8_t ) th;
  t.isIRAP = ( uint8_t ) irap; t.chromaAdj = ( uint16_t ) adj;
  return t;
}

static vtmhip_intra_chroma_joint_job jointOf( int pred, int mask, int sign, int th, int qpPer, int qpRem, int irap, int adj, int64_t outOff )
{
  vtmhip_intra_chroma_joint_job t;
  memset( &t, 0, sizeof( t ) );
  t.outOff = outOff; t.pred = pred; t.qpPer = ( int16_t ) qpPer; t.qpRem = ( int16_t ) qpRem; t.typeHor = ( uint8_t ) th; t.isIRAP = ( uint8_t ) irap;
  t.cbfMask = ( uint8_t ) mask; t.signFlag = ( uint8_t ) sign; t.chromaAdj = ( uint16_t ) adj;
  return t;
}

// 8x8 (everything available), 16x4 (above and left), 32x16 (above only, first row), 4x4 (nothing available); regular and LM jobs; 1 .. 4 single jobs and 0 .. 6 joint
// jobs per prediction
static Tables baseTables()
{
  Tables T;
  T.blocks = { blockOf( 8, 8, 10, 1, 1, 8, 8, 101 ), blockOf( 16, 4, 8, 1, 1, 0, 0, 2001 ), blockOf( 32, 16, 12, 1, 0, 16, 0, 4001 ), blockOf( 4, 4, 10, 0, 0, 0, 0, 9001 ) };
  T.blocks[2].firstRow = 1; T.blocks[1].colocated = 1;
  const int modes[][2] = { { 0, 0 }, { 0, 67 }, { 1, 1 }, { 1, 68 }, { 2, 34 }, { 2, 69 }, { 3, 66 }, { 3, 67 } };   // (block, mode)
  int64_t off = 3;
  for( const auto &m : modes )
  {
    vtmhip_intra_chroma_job j;
    memset( &j, 0, sizeof( j ) );
    const int n = T.blocks[m[0]].width * T.blocks[m[0]].height;
    j.cbPredOff = off; j.crPredOff = off + n + 5; j.block = m[0]; j.mode = ( uint8_t ) m[1];
    off += 2 * ( n + 5 );
    T.jobs.push_back( j );
  }
  const int adjs[5] = { 0, 1500, 2048, 3277, 32767 };
  int64_t out = 7;
  for( int p = 0; p < ( int ) T.jobs.size(); p++ )
  {
    const int n = T.blocks[T.jobs[p].block].width * T.blocks[T.jobs[p].block].height;
    for( int k = 0; k < 1 + p % 4; k++, out += n + 5 )
      T.tu.push_back( tuOf( p, k & 1, k & 2 ? VTMHIP_TRSKIP : VTMHIP_DCT2, 3 + p, ( p + k ) % 6, k & 1, adjs[( p + k ) % 5], out ) );
    for( int k = 0; k < p % 7; k++, out += n + 5 )
      T.joint.push_back( jointOf( p, 1 + k % 3, ( p + k ) & 1, k >= 3 ? VTMHIP_TRSKIP : VTMHIP_DCT2, 2 + p, ( p + 2 * k ) % 6, k & 1, adjs[( p + 2 * k ) % 5], out ) );
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

static bool run( const Tables &T, std::vector<vtmhip_tu_job> &outTu, std::vector<vtmhip_jccr_job> &outJoint, IchainPlan &plan )
{
  vtmhip_intra_chroma_block     *b = exact( T.blocks );
  vtmhip_intra_chroma_job       *j = exact( T.jobs );
  vtmhip_intra_chroma_tu_job    *t = exact( T.tu );
  vtmhip_intra_chroma_joint_job *q = exact( T.joint );
  vtmhip_tu_job   *o = ( vtmhip_tu_job * ) malloc( T.tu.size() * sizeof( vtmhip_tu_job ) + 1 );
  vtmhip_jccr_job *r = ( vtmhip_jccr_job * ) malloc( T.joint.size() * sizeof( vtmhip_jccr_job ) + 1 );
  memset( o, 0xa5, T.tu.size() * sizeof( vtmhip_tu_job ) );
  memset( r, 0xa5, T.joint.size() * sizeof( vtmhip_jccr_job ) );
  const bool ok = ichainMakeJobs( b, ( int ) T.blocks.size(), j, ( int ) T.jobs.size(), t, ( int ) T.tu.size(), q, ( int ) T.joint.size(), o, r, plan );
  outTu.assign( o, o + T.tu.size() );
  outJoint.assign( r, r + T.joint.size() );
  free( b ); free( j ); free( t ); free( q ); free( o ); free( r );
  return ok;
}

template<typename T> static bool untouched( const std::vector<T> &out )
{
  const unsigned char *p = ( const unsigned char * ) out.data();
  for( size_t k = 0; k < out.size() * sizeof( T ); k++ )
    if( p[k] != 0xa5 ) return false;
  return true;
}

static void test_expansion()
{
  const Tables T = baseTables();
  std::vector<vtmhip_tu_job>   outTu;
  std::vector<vtmhip_jccr_job> outJoint;
  IchainPlan plan;
  CHECK( run( T, outTu, outJoint, plan ) );
  CHECK( plan.maxBlockArea == 512 && plan.anyLm == 1 && plan.crs == 1 );
  CHECK( plan.tu.maxWidth == 32 && plan.tu.maxHeight == 16 && plan.tu.maxArea == 512 && plan.tu.uniform == 0 );
  CHECK( plan.joint.maxWidth == 32 && plan.joint.maxHeight == 16 && plan.joint.maxArea == 512 && plan.joint.uniform == 0 );
  CHECK( T.tu.size() == 20 && T.joint.size() == 21 );
  for( size_t k = 0; k < T.tu.size(); k++ )
  {
    const vtmhip_intra_chroma_tu_job &t = T.tu[k];
    const vtmhip_intra_chroma_job    &p = T.jobs[t.pred];
    const vtmhip_intra_chroma_block  &b = T.blocks[p.block];
    const vtmhip_tu_job &o = outTu[k];
    CHECK( o.resiOff == ( t.component ? p.crPredOff : p.cbPredOff ) && o.outOff == t.outOff && o.resiStride == b.width && o.width == b.width && o.height == b.height );
    CHECK( o.qpPer == t.qpPer && o.qpRem == t.qpRem && o.typeHor == t.typeHor && o.typeVer == t.typeHor && o.bitDepth == b.bitDepth && o.isIRAP == t.isIRAP );
    CHECK( o.pad == 0 && o.chromaAdj == t.chromaAdj );
  }
  for( size_t k = 0; k < T.joint.size(); k++ )
  {
    const vtmhip_intra_chroma_joint_job &t = T.joint[k];
    const vtmhip_intra_chroma_job       &p = T.jobs[t.pred];
    const vtmhip_intra_chroma_block     &b = T.blocks[p.block];
    const vtmhip_jccr_job &o = outJoint[k];
    CHECK( o.cbOff == p.cbPredOff && o.crOff == p.crPredOff && o.outOff == t.outOff && o.resiStride == b.width && o.width == b.width && o.height == b.height );
    CHECK( o.qpPer == t.qpPer && o.qpRem == t.qpRem && o.typeHor == t.typeHor && o.bitDepth == b.bitDepth && o.isIRAP == t.isIRAP );
    CHECK( o.cbfMask == t.cbfMask && o.signFlag == t.signFlag && o.chromaAdj == t.chromaAdj && o.reserved0 == 0 );
    CHECK( o.reserved1[0] == 0 && o.reserved1[1] == 0 && o.reserved1[2] == 0 && o.reserved1[3] == 0 );
  }

  // one size, DCT2 and no adj: both tables uniform, the plain chains; then transform skip / an adj in one table at a time
  Tables U;
  U.blocks = { blockOf( 8, 4, 10, 1, 1, 2, 0, 11 ), blockOf( 8, 4, 8, 0, 1, 0, 4, 301 ) };
  U.jobs = { T.jobs[0], T.jobs[2] };
  U.jobs[0].block = 0; U.jobs[1].block = 1; U.jobs[1].mode = 66;
  U.tu = { tuOf( 0, 0, VTMHIP_DCT2, 4, 0, 0, 0, 1 ), tuOf( 1, 1, VTMHIP_DCT2, 4, 5, 1, 0, 41 ) };
  U.joint = { jointOf( 1, 3, 1, VTMHIP_DCT2, 4, 1, 0, 0, 81 ) };
  CHECK( run( U, outTu, outJoint, plan ) && plan.tu.uniform == 1 && plan.joint.uniform == 1 && plan.crs == 0 && plan.anyLm == 0 && plan.maxBlockArea == 32 );
  CHECK( plan.tu.maxWidth == 8 && plan.tu.maxHeight == 4 && plan.joint.maxWidth == 8 && plan.joint.maxHeight == 4 );
  U.tu.push_back( tuOf( 0, 1, VTMHIP_TRSKIP, 4, 0, 0, 0, 121 ) );
  CHECK( run( U, outTu, outJoint, plan ) && plan.tu.uniform == 0 && plan.joint.uniform == 1 && plan.crs == 0 );
  U.tu.pop_back();
  U.joint.push_back( jointOf( 0, 1, 0, VTMHIP_TRSKIP, 4, 0, 0, 1, 121 ) );
  CHECK( run( U, outTu, outJoint, plan ) && plan.tu.uniform == 1 && plan.joint.uniform == 0 && plan.crs == 1 );
  // one table empty; the prediction pass alone; no table at all
  U.joint.clear();
  CHECK( run( U, outTu, outJoint, plan ) && plan.tu.uniform == 1 && plan.joint.uniform == 0 && plan.joint.maxWidth == 0 && plan.joint.maxArea == 0 );
  U.tu.clear();
  CHECK( run( U, outTu, outJoint, plan ) && plan.tu.uniform == 0 && plan.tu.maxWidth == 0 && plan.tu.maxHeight == 0 && plan.maxBlockArea == 32 );
  CHECK( run( Tables(), outTu, outJoint, plan ) && plan.maxBlockArea == 0 );
}

static void test_rejections()
{
  typedef std::function<void( Tables & )> Defect;
  const std::vector<Defect> defects = {
    []( Tables &T ) { T.blocks[0].width = 64; },       []( Tables &T ) { T.blocks[1].height = 2; },       []( Tables &T ) { T.blocks[3].width = 12; },
    []( Tables &T ) { T.blocks[2].bitDepth = 7; },     []( Tables &T ) { T.blocks[0].bitDepth = 13; },    []( Tables &T ) { T.blocks[1].above = 2; },
    []( Tables &T ) { T.blocks[1].left = 2; },         []( Tables &T ) { T.blocks[0].firstRow = 2; },     []( Tables &T ) { T.blocks[2].colocated = 2; },
    []( Tables &T ) { T.blocks[3].aboveRight = 2; },   []( Tables &T ) { T.blocks[3].belowLeft = 2; },    []( Tables &T ) { T.blocks[0].belowLeft = 3; },
    []( Tables &T ) { T.blocks[0].belowLeft = 10; },   []( Tables &T ) { T.blocks[0].aboveRight = -2; },  []( Tables &T ) { T.blocks[2].aboveRight = 34; },
    []( Tables &T ) { T.blocks[3].reserved[0] = 1; },  []( Tables &T ) { T.blocks[1].reserved[2] = 1; },
    []( Tables &T ) { T.jobs[1].mode = 70; },          []( Tables &T ) { T.jobs[0].mode = 255; },         []( Tables &T ) { T.jobs[1].block = 4; },
    []( Tables &T ) { T.jobs[7].block = -1; },         []( Tables &T ) { T.jobs[2].block = 1 << 30; },    []( Tables &T ) { T.jobs[3].reserved[2] = 1; },
    []( Tables &T ) { T.tu[1].pred = 8; },             []( Tables &T ) { T.tu[0].pred = -1; },            []( Tables &T ) { T.tu[3].pred = 1 << 30; },
    []( Tables &T ) { T.tu[2].component = 2; },        []( Tables &T ) { T.tu[0].typeHor = VTMHIP_DST7; }, []( Tables &T ) { T.tu[0].typeHor = VTMHIP_DCT8; },
    []( Tables &T ) { T.tu[4].typeHor = 4; },          []( Tables &T ) { T.tu[2].qpRem = 6; },            []( Tables &T ) { T.tu[2].qpRem = -1; },
    []( Tables &T ) { T.tu[4].qpPer = -1; },           []( Tables &T ) { T.tu[5].chromaAdj = 32768; },    []( Tables &T ) { T.tu[5].reserved = 1; },
    []( Tables &T ) { T.tu[6].pad = 1; },
    []( Tables &T ) { T.joint[1].pred = 8; },          []( Tables &T ) { T.joint[0].pred = -1; },         []( Tables &T ) { T.joint[3].pred = 1 << 30; },
    []( Tables &T ) { T.joint[2].cbfMask = 0; },       []( Tables &T ) { T.joint[2].cbfMask = 4; },       []( Tables &T ) { T.joint[4].signFlag = 2; },
    []( Tables &T ) { T.joint[0].typeHor = VTMHIP_DST7; }, []( Tables &T ) { T.joint[5].typeHor = 255; }, []( Tables &T ) { T.joint[6].qpRem = 6; },
    []( Tables &T ) { T.joint[6].qpRem = -1; },        []( Tables &T ) { T.joint[7].qpPer = -1; },        []( Tables &T ) { T.joint[8].chromaAdj = 65535; },
    []( Tables &T ) { T.joint[9].pad = 1; },
  };
  int rejected = 0;
  for( const Defect &d : defects )
  {
    Tables T = baseTables();
    d( T );
    std::vector<vtmhip_tu_job>   outTu;
    std::vector<vtmhip_jccr_job> outJoint;
    IchainPlan plan;
    const bool ok = run( T, outTu, outJoint, plan );
    CHECK( !ok );
    CHECK( untouched( outTu ) && untouched( outJoint ) );
    rejected += !ok;
  }
  // the largest adj and the largest availability counts are fine
  Tables T = baseTables();
  T.tu[5].chromaAdj = 32767; T.blocks[2].aboveRight = 32;
  std::vector<vtmhip_tu_job>   outTu;
  std::vector<vtmhip_jccr_job> outJoint;
  IchainPlan plan;
  CHECK( run( T, outTu, outJoint, plan ) );
  printf( "%d of %d malformed tables rejected\n", rejected, ( int ) defects.size() );
}

int main()
{
  test_expansion();
  test_rejections();
  printf( "%d failures\n", failures );
  return failures ? 1 : 0;
}
