// gen_mmvd_ref.cpp -- recording helper of tests/golden/gen_mmvd_golden.py, never part of the build: drives the reference's own MergeCtx::setMmvdMergeCandiInfo for all
// 64 MMVD indices of one CU.  Compiled by hand against the reference headers and linked to oracle/_ref/libvtmref.so (-fno-access-control: the slice's reference POC
// lists and picture pointers are set directly, where Slice::setRefPicList would have left them).
// The member reads: pu.cs->slice (POC, the two lists' reference POCs and pictures' longTerm), pu.cu->slice->getPicHeader()->getDisFracMMVD(), the merge context's
// mmvdBaseMv / mmvdUseAltHpelIf / interDirNeighbours / BcwIdx, and through PU::restrictBiPredMergeCandsOne the CU's luma size.  It writes the PU's motion and the CU's
// imv / BcwIdx.  PU::isBiPredFromDifferentDirEqDistPoc is asked on what it left.
#include <cstdlib>
#include <cstring>

#include "CommonLib/CodingStructure.h"
#include "CommonLib/ContextModelling.h"
#include "CommonLib/Picture.h"
#include "CommonLib/Rom.h"
#include "CommonLib/Slice.h"
#include "CommonLib/Unit.h"
#include "CommonLib/UnitTools.h"

template<class T> static T *zeroed() { return ( T * ) calloc( 1, sizeof( T ) ); }   // plain storage: only the fields the members read are set

// base: per base candidate 12 values -- mv0 hor, ver, mv1 hor, ver, refIdx0, refIdx1, POC of the list-0 / list-1 reference, longTerm of each, mmvdUseAltHpelIf, BcwIdx.
// out: per index 10 values -- mv0 hor, ver, mv1 hor, ver, refIdx0, refIdx1, interDir, the list-1 weight of cu.BcwIdx, imv == IMV_HPEL, isBiPredFromDifferentDirEqDistPoc
extern "C" int gen_mmvd_case( int w, int h, int curPoc, int disFrac, const int32_t *base, int32_t *out )
{
  Slice           *slice = zeroed<Slice>();
  PicHeader       *ph    = zeroed<PicHeader>();
  CodingStructure *cs    = zeroed<CodingStructure>();
  CodingUnit      *cu    = zeroed<CodingUnit>();
  PredictionUnit  *pu    = zeroed<PredictionUnit>();
  Picture         *pics[2][2];
  ph->m_disFracMMVD    = disFrac != 0;
  slice->m_pcPicHeader = ph;
  slice->m_iPOC        = curPoc;
  cs->slice            = slice;
  cu->slice            = slice;
  cu->cs               = cs;
  cu->chromaFormat     = CHROMA_400;
  cu->blocks.push_back( CompArea( COMPONENT_Y, CHROMA_400, Area( 64, 64, w, h ) ) );
  pu->cs = cs;
  pu->cu = cu;
  pu->chromaFormat = CHROMA_400;
  pu->blocks.push_back( cu->Y() );

  MergeCtx mrg;
  for( int b = 0; b < 2; b++ )
  {
    const int32_t *s = base + 12 * b;
    for( int l = 0; l < 2; l++ )
    {
      const int refIdx = s[4 + l];
      mrg.mmvdBaseMv[b][l] = MvField( refIdx >= 0 ? Mv( s[2 * l], s[2 * l + 1] ) : Mv( 0, 0 ), ( int8_t ) refIdx );
      pics[b][l] = zeroed<Picture>();
      pics[b][l]->longTerm = s[8 + l] != 0;
      pics[b][l]->poc      = s[6 + l];
      if( refIdx >= 0 )
      {
        slice->m_aiRefPOCList[l][refIdx]  = s[6 + l];
        slice->m_apcRefPicList[l][refIdx] = pics[b][l];
      }
    }
    mrg.mmvdUseAltHpelIf[b]   = s[10] != 0;
    mrg.interDirNeighbours[b] = ( unsigned char ) ( ( s[4] >= 0 ? 1 : 0 ) | ( s[5] >= 0 ? 2 : 0 ) );
    mrg.BcwIdx[b]             = ( uint8_t ) s[11];
  }
  for( int c = 0; c < 64; c++ )
  {
    mrg.setMmvdMergeCandiInfo( *pu, c );
    int32_t *o = out + 10 * c;
    o[0] = pu->mv[0].getHor(); o[1] = pu->mv[0].getVer(); o[2] = pu->mv[1].getHor(); o[3] = pu->mv[1].getVer();
    o[4] = pu->refIdx[0]; o[5] = pu->refIdx[1]; o[6] = pu->interDir;
    o[7] = getBcwWeight( cu->BcwIdx, REF_PIC_LIST_1 );
    o[8] = cu->imv == IMV_HPEL;
    o[9] = PU::isBiPredFromDifferentDirEqDistPoc( *pu );
  }
  for( int b = 0; b < 2; b++ )
    for( int l = 0; l < 2; l++ ) free( pics[b][l] );
  free( pu ); free( cu ); free( cs ); free( ph ); free( slice );
  return 0;
}
