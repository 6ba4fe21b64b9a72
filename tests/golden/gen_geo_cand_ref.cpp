// gen_geo_cand_ref.cpp -- recording helper of tests/golden/gen_geo_cand_golden.py, never part of the build: drives the reference's own members for the GEO merge
// estimation of one CU.  Compiled by hand against the reference headers and linked to oracle/_ref/libvtmref.so (-fno-access-control: m_GeoModeTest is a private
// member of EncCu).
//   gen_geo_tables   g_GeoParams, g_weightOffset and the m_GeoModeTest order of a constructed EncCu
//   gen_geo_sads     for given 14-bit candidate blocks and an original: PelBuf::roundToOutputBitdepth, the whole-block SADs and the 64 x numCand masked SADs
//                    through RdCost::setDistParam / distFunc (DF_SAD_WITH_MASK) over the reference's mask planes; where a walk starts in its plane and how it
//                    steps is the generator's arithmetic (tests/geo_util.py), passed in
//   gen_geo_sort     a list of combinations through GeoComboCostList::sortByCost; the costs and the filter are the generator's
//   gen_geo_blend    InterpolationFilter::xWeightedGeoBlk for one component of a 4:2:0 CU
//   gen_geo_dist     SATD and SAD of a block through RdCost
// Only members of the reference are called here; no step of EncCu::xCheckRDCostMergeGeo2Nx2N is restated.
#include <cstdlib>
#include <cstring>

#include "CommonLib/Buffer.h"
#include "CommonLib/InterpolationFilter.h"
#include "CommonLib/RdCost.h"
#include "CommonLib/Rom.h"
#include "CommonLib/Slice.h"
#include "CommonLib/Unit.h"
#include "EncoderLib/EncCu.h"

static void ensureRom() { if( !g_GeoParams ) initROM(); }   // once per process: initGeoTemplate allocates g_GeoParams

template<class T> static T *zeroed() { return ( T * ) calloc( 1, sizeof( T ) ); }   // plain storage: only the fields the members read are set

extern "C" int gen_geo_tables( int16_t params[GEO_NUM_PARTITION_MODE * 2], int16_t offsets[GEO_NUM_PARTITION_MODE * GEO_NUM_CU_SIZE * GEO_NUM_CU_SIZE * 2],
                               uint8_t order[GEO_MAX_NUM_CANDS * 2] )
{
  ensureRom();
  for( int s = 0; s < GEO_NUM_PARTITION_MODE; s++ )
  {
    params[2 * s] = g_GeoParams[s][0]; params[2 * s + 1] = g_GeoParams[s][1];
    for( int hIdx = 0; hIdx < GEO_NUM_CU_SIZE; hIdx++ )
      for( int wIdx = 0; wIdx < GEO_NUM_CU_SIZE; wIdx++ )
        for( int k = 0; k < 2; k++ ) offsets[( ( s * GEO_NUM_CU_SIZE + hIdx ) * GEO_NUM_CU_SIZE + wIdx ) * 2 + k] = g_weightOffset[s][hIdx][wIdx][k];
  }
  EncCu *enc = new EncCu;   // never destroyed: its cost list frees arrays that only EncCu::create allocates
  for( int i = 0; i < GEO_MAX_NUM_CANDS; i++ ) { order[2 * i] = enc->m_GeoModeTest[i].m_candIdx0; order[2 * i + 1] = enc->m_GeoModeTest[i].m_candIdx1; }
  return GEO_MAX_NUM_CANDS;
}

struct Rig
{
  Slice          *slice;
  CodingUnit     *cu;
  PredictionUnit *pu;
};

static Rig makeRig( int w, int h, int bd )
{
  Rig r;
  r.slice = zeroed<Slice>();
  r.cu    = zeroed<CodingUnit>();
  r.pu    = zeroed<PredictionUnit>();
  for( int c = 0; c < 3; c++ )
  {
    r.slice->m_clpRngs.comp[c].min = 0;
    r.slice->m_clpRngs.comp[c].max = ( 1 << bd ) - 1;
    r.slice->m_clpRngs.comp[c].bd  = bd;
  }
  const UnitArea ua( CHROMA_420, Area( 0, 0, w, h ) );
  r.cu->UnitArea::operator=( ua );
  r.pu->UnitArea::operator=( ua );
  r.cu->chromaFormat = CHROMA_420;
  r.pu->chromaFormat = CHROMA_420;
  r.cu->slice        = r.slice;
  r.pu->cu           = r.cu;
  return r;
}
static void freeRig( Rig &r ) { free( r.pu ); free( r.cu ); free( r.slice ); }

// comp 0: w x h luma samples; 1 / 2: ( w / 2 ) x ( h / 2 ); every block with stride = its width
extern "C" int gen_geo_blend( int w, int h, int bd, int splitDir, int comp, const int16_t *src0, const int16_t *src1, int16_t *dst )
{
  ensureRom();
  Rig       r  = makeRig( w, h, bd );
  const int bw = comp ? w / 2 : w, bh = comp ? h / 2 : h;
  auto      mk = [&]( const int16_t *p ) {
    PelBuf b( const_cast<Pel *>( p ), bw, bw, bh );
    return PelUnitBuf( CHROMA_420, comp == 0 ? b : PelBuf(), comp == 1 ? b : PelBuf(), comp == 2 ? b : PelBuf() );
  };
  PelUnitBuf a = mk( src0 ), b = mk( src1 ), d = mk( dst );
  InterpolationFilter::xWeightedGeoBlk( *r.pu, bw, bh, ComponentID( comp ), uint8_t( splitDir ), d, a, b );
  freeRig( r );
  return 0;
}

// The rounded copies of numCand 14-bit blocks (PelBuf::roundToOutputBitdepth), their SADs against the original and their masked SADs for 64 walks over the
// reference's mask planes, all through RdCost::setDistParam / distFunc.  walk[s] = { plane, first entry, maskStride, stepX, maskStride2 }: the caller's arithmetic.
extern "C" int gen_geo_sads( int w, int h, int bd, int numCand, const int16_t *org, const int16_t *const pred[6], const int32_t walk[GEO_NUM_PARTITION_MODE][5],
                             uint64_t sadWhole[6], uint64_t sadLarge[GEO_NUM_PARTITION_MODE * 6] )
{
  ensureRom();
  static RdCost rd;
  Rig           r = makeRig( w, h, bd );
  const CPelBuf orgBuf( org, w, w, h );
  Pel          *rounded = ( Pel * ) malloc( sizeof( Pel ) * w * h );
  for( int c = 0; c < numCand; c++ )
  {
    PelBuf dst( rounded, w, w, h );
    dst.copyFrom( CPelBuf( pred[c], w, w, h ) );
    dst.roundToOutputBitdepth( dst, r.slice->m_clpRngs.comp[0] );
    DistParam whole;
    rd.setDistParam( whole, orgBuf, rounded, w, bd, COMPONENT_Y );
    sadWhole[c] = whole.distFunc( whole );
    for( int s = 0; s < GEO_NUM_PARTITION_MODE; s++ )
    {
      DistParam masked;
      rd.setDistParam( masked, orgBuf, rounded, w, g_globalGeoEncSADmask[walk[s][0]] + walk[s][1], walk[s][2], walk[s][3], walk[s][4], bd, COMPONENT_Y );
      sadLarge[s * 6 + c] = masked.distFunc( masked );
    }
  }
  free( rounded );
  freeRig( r );
  return 0;
}

// n rows of ( splitDir, cand0, cand1 ) with their costs, in the order the caller appended them, through a GeoComboCostList and its own sortByCost, in place
extern "C" int gen_geo_sort( int n, int32_t *rows, double *cost )
{
  GeoComboCostList l;
  for( int i = 0; i < n; i++ ) l.list.push_back( GeoMergeCombo( rows[3 * i], rows[3 * i + 1], rows[3 * i + 2], cost[i] ) );
  if( n ) l.sortByCost();
  for( int i = 0; i < n; i++ )
  {
    rows[3 * i] = l.list[i].splitDir; rows[3 * i + 1] = l.list[i].mergeIdx0; rows[3 * i + 2] = l.list[i].mergeIdx1;
    cost[i] = l.list[i].cost;
  }
  return n;
}

// SATD and SAD of a w x h luma block against the original, through RdCost::setDistParam / distFunc
extern "C" int gen_geo_dist( int w, int h, int bd, const int16_t *org, const int16_t *cur, uint64_t out[2] )
{
  static RdCost rd;
  for( int hadamard = 0; hadamard < 2; hadamard++ )
  {
    DistParam dp;
    rd.setDistParam( dp, CPelBuf( org, w, w, h ), CPelBuf( cur, w, w, h ), bd, COMPONENT_Y, hadamard != 0 );
    out[hadamard ? 0 : 1] = dp.distFunc( dp );
  }
  return 0;
}
