// gen_lfnst_mode_ref.cpp -- recording helper of tests/golden/gen_lfnst_mode_golden.py, never part of the build: asks the reference which LFNST transform set and
// transpose flag a regular luma mode gets on a W x H transform unit.  Compiled by hand against the reference headers and linked to oracle/_ref/libvtmref.so
// (-fno-access-control: the two TrQuant members are not public):
//   PU::getWideAngle                -> the wide-angle mode, on a TransformUnit that holds only what the function reads (its luma block and a CodingUnit without ISP)
//   TrQuant::getLFNSTIntraMode      -> the index into g_lfnstLut          (the real members of a default-constructed TrQuant, not restatements)
//   TrQuant::getTransposeFlag
// gen_lfnst_lut copies g_lfnstLut out of CommonLib/RomLFNST.cpp.
#include <cstdlib>
#include <cstring>

#include "CommonLib/Rom.h"
#include "CommonLib/TrQuant.h"
#include "CommonLib/Unit.h"
#include "CommonLib/UnitTools.h"

template<class T> static T *zeroed() { return ( T * ) calloc( 1, sizeof( T ) ); }   // plain storage: only the fields PU::getWideAngle reads are set

extern "C" int gen_lfnst_lut( uint8_t *lut )
{
  memcpy( lut, g_lfnstLut, sizeof( g_lfnstLut ) );
  return ( int ) sizeof( g_lfnstLut );
}

// out: wide-angle mode, g_lfnstLut[ getLFNSTIntraMode( . ) ], getTransposeFlag( . )
extern "C" int gen_lfnst_mode( int w, int h, int mode, int32_t *out )
{
  static TrQuant trQuant;
  CodingUnit    *cu = zeroed<CodingUnit>();
  TransformUnit *tu = zeroed<TransformUnit>();
  const CompArea area( COMPONENT_Y, CHROMA_420, Area( 0, 0, w, h ) );
  cu->chromaFormat = CHROMA_420;
  cu->blocks.push_back( area );
  cu->ispMode = 0;
  tu->chromaFormat = CHROMA_420;
  tu->blocks.push_back( area );
  tu->cu = cu;
  const int      wide      = PU::getWideAngle( *tu, ( uint32_t ) mode, COMPONENT_Y );
  const uint32_t intraMode = trQuant.getLFNSTIntraMode( wide );
  out[0] = wide;
  out[1] = g_lfnstLut[intraMode];
  out[2] = trQuant.getTransposeFlag( intraMode ) ? 1 : 0;
  free( tu ); free( cu );
  return 0;
}
