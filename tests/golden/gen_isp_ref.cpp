// gen_isp_ref.cpp -- recording helper of tests/golden/gen_isp_golden.py, never part of the build: drives the reference's own IntraPrediction members for the
// prediction regions of one ISP CU.  Compiled by hand against the reference headers and linked to oracle/_ref/libvtmref.so (-fno-access-control: the chosen lines are
// placed straight into the object's reference buffers, where xFillReferenceSamples would have left them for the first sub-partition):
//   initPredIntraParams        with cu->ispMode set and the CU block different from the area  -> m_ipaParam (region 0)
//   initIntraPatternChTypeISP  for every region behind the first, on a reconstruction the caller chose  -> the two lines it leaves, and m_ipaParam
//   predIntraAng               on every region -> its prediction
// The availability branch of initIntraPatternChTypeISP asks cs.getCURestricted / cs.isDecomp for the position left of (horizontal split) or above (vertical split)
// the region: the CU lives in a small real CodingStructure, and `sideAvail` adds a neighbour CU on that side and marks it decomposed; without it the position holds no
// CU and the member takes its other branch.
#include <cstdlib>
#include <cstring>

#include "CommonLib/CodingStructure.h"
#include "CommonLib/IntraPrediction.h"
#include "CommonLib/Slice.h"
#include "CommonLib/Unit.h"

template<class T> static T *zeroed() { return ( T * ) calloc( 1, sizeof( T ) ); }   // plain storage: only the fields the members read are set

enum { CU_X = 64, CU_Y = 64, CS_SIZE = 256, MAX_LINE = 129 };

// top: 2W + 1, left: 2H + 1 samples; reco: W x H (stride W), read next to the regions behind the first.
// pred: the assembled W x H prediction; params: 8 per region; linesOut: per region behind the first MAX_LINE top samples, then MAX_LINE left samples (the first
// cuW + regW + 1 and cuH + regH + 1 of each are what the member leaves defined)
extern "C" int gen_isp_case( int w, int h, int mode, int split, int sideAvail, int bd, int regW, int regH, const int16_t *top, const int16_t *left, const int16_t *reco,
                             int16_t *pred, int32_t *params, int16_t *linesOut )
{
  static IntraPrediction ip;
  static SPS             sps;
  static CUCache         cuCache;
  static PUCache         puCache;
  static TUCache         tuCache;
  sps.setMaxCUWidth( 128 );
  sps.setMaxCUHeight( 128 );
  Slice *slice = zeroed<Slice>();
  slice->m_clpRngs.comp[COMPONENT_Y].min = 0;
  slice->m_clpRngs.comp[COMPONENT_Y].max = ( 1 << bd ) - 1;
  slice->m_clpRngs.comp[COMPONENT_Y].bd  = bd;
  slice->setSPS( &sps );

  CodingStructure *cs = new CodingStructure( cuCache, puCache, tuCache );
  cs->create( CHROMA_400, Area( 0, 0, CS_SIZE, CS_SIZE ), true, false );
  cs->slice = slice;
  cs->sps   = &sps;
  if( sideAvail )
  {
    const Area nb = split == HOR_INTRA_SUBPARTITIONS ? Area( CU_X - 8, CU_Y, 8, h ) : Area( CU_X, CU_Y - 8, w, 8 );
    CodingUnit &n = cs->addCU( UnitArea( CHROMA_400, nb ), CHANNEL_TYPE_LUMA );
    n.slice = slice;
    n.tileIdx = 0;
    cs->setDecomp( n.Y() );
  }
  CodingUnit &cu = cs->addCU( UnitArea( CHROMA_400, Area( CU_X, CU_Y, w, h ) ), CHANNEL_TYPE_LUMA );
  cu.slice   = slice;
  cu.tileIdx = 0;
  cu.ispMode = split;
  PredictionUnit *pu = zeroed<PredictionUnit>();
  pu->cs = cs;
  pu->cu = &cu;
  pu->chromaFormat = CHROMA_400;
  pu->blocks.push_back( cu.Y() );
  pu->intraDir[CHANNEL_TYPE_LUMA] = mode;
  pu->multiRefIdx = 0;
  cu.firstPU = pu;

  const int predStride = 2 * w + 1;
  ip.m_refBufferStride[COMPONENT_Y] = predStride;
  Pel *unfiltered = ip.m_refBuffer[COMPONENT_Y][PRED_BUF_UNFILTERED];
  memset( unfiltered, 0x55, sizeof( ip.m_refBuffer[COMPONENT_Y][PRED_BUF_UNFILTERED] ) );
  memset( ip.m_refBuffer[COMPONENT_Y][PRED_BUF_FILTERED], 0x55, sizeof( ip.m_refBuffer[COMPONENT_Y][PRED_BUF_FILTERED] ) );
  memcpy( unfiltered, top, sizeof( Pel ) * ( 2 * w + 1 ) );
  memcpy( unfiltered + predStride, left, sizeof( Pel ) * ( 2 * h + 1 ) );

  const int numRegions = split == HOR_INTRA_SUBPARTITIONS ? h / regH : w / regW;
  for( int r = 0; r < numRegions; r++ )
  {
    const int      rx = split == HOR_INTRA_SUBPARTITIONS ? 0 : r * regW, ry = split == HOR_INTRA_SUBPARTITIONS ? r * regH : 0;
    const CompArea area( COMPONENT_Y, CHROMA_400, Area( CU_X + rx, CU_Y + ry, regW, regH ) );
    ip.m_ipaParam = IntraPrediction::IntraPredParam();
    if( r == 0 )
    {
      // what initIntraPatternChTypeISP does for the first sub-partition, without the fetch of the CU's samples from a picture
      ip.initPredIntraParams( *pu, area, sps );
      ip.m_topRefLength  = w + regW;
      ip.m_leftRefLength = h + regH;
    }
    else
    {
      PelBuf rec( const_cast<int16_t *>( reco ) + ry * w + rx, w, regW, regH );
      ip.initIntraPatternChTypeISP( cu, area, rec );
      int16_t *lo = linesOut + ( r - 1 ) * 2 * MAX_LINE;
      memcpy( lo, unfiltered, sizeof( Pel ) * ( w + regW + 1 ) );
      memcpy( lo + MAX_LINE, unfiltered + predStride, sizeof( Pel ) * ( h + regH + 1 ) );
    }
    if( ip.m_ipaParam.refFilterFlag ) return -1;   // never under ISP
    PelBuf dst( pred + ry * w + rx, w, regW, regH );
    ip.predIntraAng( COMPONENT_Y, dst, *pu );
    int32_t *p = params + 8 * r;
    p[0] = IntraPrediction::getModifiedWideAngle( w, h, mode );
    p[1] = ip.m_ipaParam.isModeVer;
    p[2] = ip.m_ipaParam.intraPredAngle;
    p[3] = ip.m_ipaParam.invAngle;
    p[4] = ip.m_ipaParam.angularScale;
    p[5] = ip.m_ipaParam.applyPDPC;
    p[6] = ip.m_ipaParam.refFilterFlag;
    p[7] = ip.m_ipaParam.interpolationFlag;
  }
  free( pu );
  cs->destroy();
  delete cs;
  free( slice );
  return 0;
}
