// gen_intra_ref.cpp -- recording helper of tests/golden/gen_intra_golden.py, never part of the build: drives the reference's own IntraPrediction members for one luma
// block.  Compiled by hand against the reference headers and linked to oracle/_ref/libvtmref.so (-fno-access-control: the chosen lines are placed straight into the
// object's reference buffers, where xFillReferenceSamples would have left them):
//   initPredIntraParams  -> m_ipaParam          (the real member, not a restatement)
//   xFilterReferenceSamples                     (when m_ipaParam.refFilterFlag, as initIntraPatternChType does)
//   predIntraAng         -> the prediction, PDPC included
#include <cstdlib>
#include <cstring>

#include "CommonLib/CodingStructure.h"
#include "CommonLib/IntraPrediction.h"
#include "CommonLib/Slice.h"
#include "CommonLib/Unit.h"

template<class T> static T *zeroed() { return ( T * ) calloc( 1, sizeof( T ) ); }   // plain storage: only the fields the three members read are set

extern "C" int gen_intra_case( int w, int h, int mode, int m, int bd, const int16_t *top, const int16_t *left, int16_t *pred, int32_t *params )
{
  static IntraPrediction ip;
  static SPS             sps;
  CodingStructure *cs    = zeroed<CodingStructure>();
  Slice           *slice = zeroed<Slice>();
  CodingUnit      *cu    = zeroed<CodingUnit>();
  PredictionUnit  *pu    = zeroed<PredictionUnit>();
  slice->m_clpRngs.comp[COMPONENT_Y].min = 0;
  slice->m_clpRngs.comp[COMPONENT_Y].max = ( 1 << bd ) - 1;
  slice->m_clpRngs.comp[COMPONENT_Y].bd  = bd;
  cs->slice = slice;
  const CompArea area( COMPONENT_Y, CHROMA_420, Area( 0, 0, w, h ) );
  cu->cs = cs;
  cu->chromaFormat = CHROMA_420;
  cu->blocks.push_back( area );
  pu->cs = cs;
  pu->cu = cu;
  pu->chromaFormat = CHROMA_420;
  pu->blocks.push_back( area );
  pu->intraDir[CHANNEL_TYPE_LUMA] = mode;
  pu->multiRefIdx = m;

  const int predStride = 2 * w + 1 + m;
  ip.m_topRefLength  = 2 * w;
  ip.m_leftRefLength = 2 * h;
  ip.m_refBufferStride[COMPONENT_Y] = predStride;
  Pel *unfiltered = ip.m_refBuffer[COMPONENT_Y][PRED_BUF_UNFILTERED], *filtered = ip.m_refBuffer[COMPONENT_Y][PRED_BUF_FILTERED];
  memset( unfiltered, 0x55, sizeof( ip.m_refBuffer[COMPONENT_Y][PRED_BUF_UNFILTERED] ) );
  memset( filtered, 0x55, sizeof( ip.m_refBuffer[COMPONENT_Y][PRED_BUF_FILTERED] ) );
  memcpy( unfiltered, top, sizeof( Pel ) * ( 2 * w + 1 + m ) );
  memcpy( unfiltered + predStride, left, sizeof( Pel ) * ( 2 * h + 1 + m ) );

  ip.m_ipaParam = IntraPrediction::IntraPredParam();
  ip.initPredIntraParams( *pu, area, sps );
  if( ip.m_ipaParam.refFilterFlag ) ip.xFilterReferenceSamples( unfiltered, filtered, area, sps, m );
  PelBuf dst( pred, w, w, h );
  ip.predIntraAng( COMPONENT_Y, dst, *pu );

  params[0] = IntraPrediction::getModifiedWideAngle( w, h, mode );
  params[1] = ip.m_ipaParam.isModeVer;
  params[2] = ip.m_ipaParam.intraPredAngle;
  params[3] = ip.m_ipaParam.invAngle;
  params[4] = ip.m_ipaParam.angularScale;
  params[5] = ip.m_ipaParam.applyPDPC;
  params[6] = ip.m_ipaParam.refFilterFlag;
  params[7] = ip.m_ipaParam.interpolationFlag;
  params[8] = ip.m_ipaParam.multiRefIndex;
  free( pu ); free( cu ); free( slice ); free( cs );
  return 0;
}
