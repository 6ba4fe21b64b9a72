// gen_cclm_ref.cpp -- recording helper of tests/golden/gen_cclm_golden.py, never part of the build: drives the reference's own IntraPrediction members for one
// 4:2:0 CU on a small real Picture / CodingStructure.  Compiled by hand against the reference headers and linked to oracle/_ref/libvtmref.so
// (-fno-access-control).  Availability is what the reference finds: the picture edge, the CTU row, and the neighbouring CUs this helper has added and marked
// decoded before the current one.
//   initIntraPatternChType (Cb, Cr)  -> the unfiltered reference lines (xFillReferenceSamples from the chroma reconstruction planes)
//   xGetLumaRecPixels                -> the down-sampled luma, LM extent (m_piTemp) and MDLM extent (m_pMdlmTemp)
//   xGetLMParameters                 -> (a, b, shift) per component and LM mode
//   predIntraChromaLM                -> the LM predictions
//   initPredIntraParams / predIntraAng (Cb, Cr) -> the regular predictions
//   CodingStructure::isDecomp / getCURestricted, walked as isAboveAvailable & co. walk them -> the flags and counts stored beside the block
#include <cstdlib>
#include <cstring>
#include <new>

#include "CommonLib/CodingStructure.h"
#include "CommonLib/IntraPrediction.h"
#include "CommonLib/Picture.h"
#include "CommonLib/Slice.h"
#include "CommonLib/Unit.h"
#include "CommonLib/UnitTools.h"

// the reference's availability walks (IntraPrediction.cpp:1215-1320; file-local there, not exported by the library) over the real CodingStructure members: units from
// `start` in steps of (dx, dy), stopping at the first position that is not decoded, counting the ones whose CU precedes the current one in its slice and tile
static int availableUnits( const CodingUnit &cu, Position start, int dx, int dy, int numUnits )
{
  const CodingStructure &cs = *cu.cs;
  int n = 0;
  for( int i = 0; i < numUnits; i++ )
  {
    const Position refPos = start.offset( i * dx, i * dy );
    if( !cs.isDecomp( refPos, CHANNEL_TYPE_CHROMA ) ) break;
    if( cs.getCURestricted( refPos, cu, CHANNEL_TYPE_CHROMA ) != nullptr ) n++;
  }
  return n;
}

template<class T, class... A> static T *zeroNew( A &&... a ) { void *m = calloc( 1, sizeof( T ) ); return new( m ) T( std::forward<A>( a )... ); }

struct GenCclmIn
{
  int32_t picW, picH, ctuSize, bitDepth, colocated;
  int32_t x, y, w, h;            // the CU, luma samples
  int32_t numNbr;                // neighbouring CUs added (and marked decoded) before it
  int32_t nbr[16][4];            // luma x, y, w, h
  int32_t numModes;
  int32_t modes[70];             // the regular modes to predict
  int16_t *luma, *cb, *cr;       // the reconstruction planes, stride picW and picW / 2
};

struct GenCclmOut
{
  int32_t  avail[4];             // above, left, available above-right / below-left chroma samples
  int32_t  firstRow;
  int16_t *lines;                // Cb top (2W + 1), Cb left (2H + 1), Cr top, Cr left
  int16_t *dsLm, *dsMdlm;        // each: inner W x H, then the top row of 2W, then the left column of 2H samples as the member left them (beyond the filled part: whatever the buffer held)
  int32_t *params;               // [3 modes 67 .. 69][2][a, b, shift]
  int16_t *predLm;               // [3][2][H][W]
  int16_t *predReg;              // [numModes][2][H][W]
};

extern "C" int gen_cclm_case( const GenCclmIn *in, GenCclmOut *out )
{
  static bool rom = false;
  if( !rom ) { initROM(); rom = true; }
  IntraPrediction *ip = new IntraPrediction();
  ip->init( CHROMA_420, in->bitDepth );
  SPS   *sps   = new SPS();
  PPS   *pps   = new PPS();
  Slice *slice = zeroNew<Slice>();
  sps->setChromaFormatIdc( CHROMA_420 );
  sps->setMaxCUWidth( in->ctuSize );
  sps->setMaxCUHeight( in->ctuSize );
  sps->setBitDepth( CHANNEL_TYPE_LUMA, in->bitDepth );
  sps->setBitDepth( CHANNEL_TYPE_CHROMA, in->bitDepth );
  sps->setVerCollocatedChromaFlag( in->colocated != 0 );   // = sps_cclm_colocated_chroma_flag (getCclmCollocatedChromaFlag)
  sps->setEntropyCodingSyncEnabledFlag( false );
  pps->setPicWidthInLumaSamples( in->picW );
  pps->setPicHeightInLumaSamples( in->picH );
  PreCalcValues *pcv = new PreCalcValues( *sps, *pps, true );
  slice->setSPS( sps );
  slice->setPPS( pps );
  for( int c = 0; c < 3; c++ )
  {
    slice->m_clpRngs.comp[c].min = 0;
    slice->m_clpRngs.comp[c].max = ( 1 << in->bitDepth ) - 1;
    slice->m_clpRngs.comp[c].bd  = in->bitDepth;
  }

  static CUCache cuCache;
  static PUCache puCache;
  static TUCache tuCache;
  CodingStructure *cs  = zeroNew<CodingStructure>( cuCache, puCache, tuCache );
  Picture         *pic = zeroNew<Picture>();
  cs->create( CHROMA_420, Area( 0, 0, in->picW, in->picH ), true, false );
  cs->sps = sps; cs->pps = pps; cs->slice = slice; cs->pcv = pcv; cs->picture = pic;
  cs->initStructData( 32, true );
  for( int i = 0; i < 2; i++ ) memset( cs->m_isDecomp[i], 0, sizeof( bool ) * cs->unitScale[i].scale( cs->area.blocks[i].size() ).area() );
  pic->chromaFormat = CHROMA_420;
  pic->cs = cs;
  pic->m_bufs[PIC_RECONSTRUCTION].createFromBuf( PelUnitBuf( CHROMA_420, PelBuf( in->luma, in->picW, in->picW, in->picH ), PelBuf( in->cb, in->picW / 2, in->picW / 2, in->picH / 2 ),
                                                             PelBuf( in->cr, in->picW / 2, in->picW / 2, in->picH / 2 ) ) );
  for( int i = 0; i < in->numNbr; i++ )
  {
    const UnitArea ua( CHROMA_420, Area( in->nbr[i][0], in->nbr[i][1], in->nbr[i][2], in->nbr[i][3] ) );
    CodingUnit &n = cs->addCU( ua, CHANNEL_TYPE_LUMA );
    n.slice = slice; n.tileIdx = 0; n.predMode = MODE_INTRA;
    cs->setDecomp( ua );
  }
  const UnitArea ua( CHROMA_420, Area( in->x, in->y, in->w, in->h ) );
  CodingUnit &cu = cs->addCU( ua, CHANNEL_TYPE_LUMA );
  cu.slice = slice; cu.tileIdx = 0; cu.predMode = MODE_INTRA;
  PredictionUnit &pu = cs->addPU( ua, CHANNEL_TYPE_LUMA );
  pu.intraDir[0] = DC_IDX;
  pu.multiRefIdx = 0;

  const CompArea areaCb = pu.Cb(), areaCr = pu.Cr();
  const int      W = areaCb.width, H = areaCb.height;
  // the flags and counts, by the reference's own walks over the chroma units
  {
    const int unit = 2, aboveUnits = W / unit, leftUnits = H / unit;
    const Position lt = areaCb.pos();
    out->avail[0] = availableUnits( cu, lt.offset( 0, -1 ), unit, 0, aboveUnits ) == aboveUnits;
    out->avail[1] = availableUnits( cu, lt.offset( -1, 0 ), 0, unit, leftUnits ) == leftUnits;
    out->avail[2] = out->avail[0] ? unit * availableUnits( cu, lt.offset( W, -1 ), unit, 0, aboveUnits ) : 0;
    out->avail[3] = out->avail[1] ? unit * availableUnits( cu, lt.offset( -1, H ), 0, unit, leftUnits ) : 0;
    out->firstRow = ( in->y & ( in->ctuSize - 1 ) ) == 0;
  }

  pu.intraDir[1] = MDLM_L_IDX;
  int16_t *line = out->lines;
  for( int c = 1; c < 3; c++ )
  {
    ip->initIntraPatternChType( cu, c == 1 ? areaCb : areaCr );
    const Pel *u = ip->m_refBuffer[c][PRED_BUF_UNFILTERED];
    memcpy( line, u, sizeof( Pel ) * ( 2 * W + 1 ) );
    memcpy( line + 2 * W + 1, u + ip->m_refBufferStride[c], sizeof( Pel ) * ( 2 * H + 1 ) );
    line += 2 * W + 1 + 2 * H + 1;
  }
  for( int k = 0; k < 3; k++ )
  {
    const int mode = k == 0 ? MDLM_L_IDX : k == 1 ? MDLM_T_IDX : LM_CHROMA_IDX;
    pu.intraDir[1] = mode;
    if( k != 1 )   // one down-sampling serves both MDLM modes, as estIntraPredChromaQT runs it
    {
      const bool mdlm   = mode != LM_CHROMA_IDX;
      const int  stride = mdlm ? 2 * MAX_CU_SIZE + 1 : MAX_CU_SIZE + 1;
      Pel       *t      = mdlm ? ip->m_pMdlmTemp : ip->m_piTemp;
      for( int i = 0; i < stride * ( 2 * H + 2 ) && i < ( mdlm ? ( 2 * MAX_CU_SIZE + 1 ) * ( 2 * MAX_CU_SIZE + 1 ) : ( MAX_CU_SIZE + 1 ) * ( MAX_CU_SIZE + 1 ) ); i++ ) t[i] = 0x5555;
      ip->xGetLumaRecPixels( pu, areaCb );
      const Pel *d0 = t + stride + 1;
      int16_t   *o  = mdlm ? out->dsMdlm : out->dsLm;
      for( int y = 0; y < H; y++ ) memcpy( o + y * W, d0 + y * stride, sizeof( Pel ) * W );
      const int nT = mdlm ? 2 * W : W, nL = mdlm ? 2 * H : H;
      for( int i = 0; i < 2 * W; i++ ) o[W * H + i] = i < nT ? d0[i - stride] : 0x5555;
      for( int j = 0; j < 2 * H; j++ ) o[W * H + 2 * W + j] = j < nL ? d0[j * stride - 1] : 0x5555;
    }
    const int slot = mode - LM_CHROMA_IDX;
    for( int c = 1; c < 3; c++ )
    {
      int a, b, shift;
      ip->xGetLMParameters( pu, ComponentID( c ), c == 1 ? areaCb : areaCr, a, b, shift );
      int32_t *p = out->params + ( slot * 2 + c - 1 ) * 3;
      p[0] = a; p[1] = b; p[2] = shift;
      PelBuf dst( out->predLm + ( slot * 2 + c - 1 ) * W * H, W, W, H );
      ip->predIntraChromaLM( ComponentID( c ), dst, pu, c == 1 ? areaCb : areaCr, mode );
    }
  }
  for( int k = 0; k < in->numModes; k++ )
  {
    pu.intraDir[1] = in->modes[k];
    for( int c = 1; c < 3; c++ )
    {
      ip->initPredIntraParams( pu, c == 1 ? areaCb : areaCr, *sps );
      PelBuf dst( out->predReg + ( k * 2 + c - 1 ) * W * H, W, W, H );
      ip->predIntraAng( ComponentID( c ), dst, pu );
    }
  }
  return 0;   // the objects of one case are left to the process: a recording run is short
}
