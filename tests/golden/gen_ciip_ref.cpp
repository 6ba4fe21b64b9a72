// gen_ciip_ref.cpp -- recording helper of tests/golden/gen_ciip_golden.py, never part of the build: drives the reference's own IntraPrediction members for one CIIP
// CU.  Compiled by hand against the reference headers and linked to oracle/_ref/libvtmref.so (-fno-access-control: the chosen lines are placed straight into the
// object's reference buffers, where xFillReferenceSamples would have left them -- the fetch of samples from a picture is the one step of initIntraPatternChType
// that is not run; the rest of it is: initPredIntraParams, setReferenceArrayLengths' lengths, xFilterReferenceSamples where refFilterFlag asks for it):
//   initPredIntraParams + xFilterReferenceSamples + predIntraAng   with pu.ciipFlag set, planar luma, DM_CHROMA chroma   -> the intra block of Y, Cb, Cr
//   geneWeightedPred                                               on an inter block the caller chose                     -> the blended block of Y, Cb, Cr
// geneWeightedPred asks cs.getPURestricted for the PUs left of the bottom-left sample and above the top-right sample: the CU lives in a small real CodingStructure
// (4:2:0), and leftKind / aboveKind add a neighbour CU with its PU on that side: 0 none, 1 inter, 2 intra.
#include <cstdlib>
#include <cstring>

#include "CommonLib/CodingStructure.h"
#include "CommonLib/IntraPrediction.h"
#include "CommonLib/Slice.h"
#include "CommonLib/Unit.h"
#include "CommonLib/UnitTools.h"

template<class T> static T *zeroed() { return ( T * ) calloc( 1, sizeof( T ) ); }   // plain storage: only the fields the members read are set

enum { CU_X = 64, CU_Y = 64, CS_SIZE = 256 };

static void addNeighbour( CodingStructure *cs, Slice *slice, const Area &a, int kind )
{
  const UnitArea ua( CHROMA_420, a );
  CodingUnit    &n = cs->addCU( ua, CHANNEL_TYPE_LUMA );
  n.slice    = slice;
  n.tileIdx  = 0;
  n.predMode = kind == 2 ? MODE_INTRA : MODE_INTER;
  cs->addPU( ua, CHANNEL_TYPE_LUMA );
  cs->setDecomp( ua );
}

// lines[c]: top (2 Wc + 1) then left (2 Hc + 1) of component c; inter[c], intra[c], blend[c]: Wc x Hc, stride Wc.  Components whose width is 2 are left alone
// (the reference keeps the inter chroma there).  info[c]: refFilterFlag | applyPDPC << 1 | final intra mode << 8.
extern "C" int gen_ciip_case( int w, int h, int bd, int leftKind, int aboveKind, const int16_t *const lines[3], const int16_t *const inter[3], int16_t *const intra[3],
                              int16_t *const blend[3], int32_t info[3] )
{
  static IntraPrediction ip;
  static SPS             sps;
  static CUCache         cuCache;
  static PUCache         puCache;
  static TUCache         tuCache;
  sps.setMaxCUWidth( 128 );
  sps.setMaxCUHeight( 128 );
  sps.setChromaFormatIdc( CHROMA_420 );
  Slice *slice = zeroed<Slice>();
  for( int c = 0; c < 3; c++ )
  {
    slice->m_clpRngs.comp[c].min = 0;
    slice->m_clpRngs.comp[c].max = ( 1 << bd ) - 1;
    slice->m_clpRngs.comp[c].bd  = bd;
  }
  slice->setSPS( &sps );

  CodingStructure *cs = new CodingStructure( cuCache, puCache, tuCache );
  cs->create( CHROMA_420, Area( 0, 0, CS_SIZE, CS_SIZE ), true, false );
  cs->slice = slice;
  cs->sps   = &sps;
  if( leftKind ) addNeighbour( cs, slice, Area( CU_X - 8, CU_Y, 8, h ), leftKind );
  if( aboveKind ) addNeighbour( cs, slice, Area( CU_X, CU_Y - 8, w, 8 ), aboveKind );
  const UnitArea ua( CHROMA_420, Area( CU_X, CU_Y, w, h ) );
  CodingUnit    &cu = cs->addCU( ua, CHANNEL_TYPE_LUMA );
  cu.slice    = slice;
  cu.tileIdx  = 0;
  cu.predMode = MODE_INTER;
  PredictionUnit &pu = cs->addPU( ua, CHANNEL_TYPE_LUMA );
  pu.ciipFlag    = true;
  pu.mergeFlag   = true;
  pu.multiRefIdx = 0;
  pu.intraDir[CHANNEL_TYPE_LUMA]   = PLANAR_IDX;
  pu.intraDir[CHANNEL_TYPE_CHROMA] = DM_CHROMA_IDX;

  int status = 0;
  for( int c = 0; c < 3; c++ )
  {
    const ComponentID compID = ComponentID( c );
    const CompArea   &area   = pu.blocks[c];
    const int         cw = area.width, ch = area.height;
    info[c] = -1;
    if( cw == 2 ) continue;
    const int predStride = 2 * cw + 1;
    Pel      *unfiltered = ip.m_refBuffer[c][PRED_BUF_UNFILTERED], *filtered = ip.m_refBuffer[c][PRED_BUF_FILTERED];
    memset( unfiltered, 0x55, sizeof( ip.m_refBuffer[c][PRED_BUF_UNFILTERED] ) );
    memset( filtered, 0x55, sizeof( ip.m_refBuffer[c][PRED_BUF_FILTERED] ) );
    memcpy( unfiltered, lines[c], sizeof( Pel ) * ( 2 * cw + 1 ) );
    memcpy( unfiltered + predStride, lines[c] + 2 * cw + 1, sizeof( Pel ) * ( 2 * ch + 1 ) );
    // initIntraPatternChType without the fetch
    ip.m_ipaParam = IntraPrediction::IntraPredParam();
    ip.initPredIntraParams( pu, area, sps );
    ip.m_refBufferStride[c] = predStride;
    ip.m_topRefLength       = 2 * cw;
    ip.m_leftRefLength      = 2 * ch;
    if( ip.m_ipaParam.refFilterFlag ) ip.xFilterReferenceSamples( unfiltered, filtered, area, sps, pu.multiRefIdx );
    PelBuf dst( intra[c], cw, cw, ch );
    ip.predIntraAng( compID, dst, pu );
    info[c] = ( ip.m_ipaParam.refFilterFlag ? 1 : 0 ) | ( ip.m_ipaParam.applyPDPC ? 2 : 0 ) | ( int ) ( PU::getFinalIntraMode( pu, toChannelType( compID ) ) << 8 );
    memcpy( blend[c], inter[c], sizeof( Pel ) * cw * ch );
    PelBuf mix( blend[c], cw, cw, ch );
    ip.geneWeightedPred( compID, mix, pu, intra[c] );
  }
  cs->destroy();
  delete cs;
  free( slice );
  return status;
}
