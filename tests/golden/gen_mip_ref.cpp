// gen_mip_ref.cpp -- recording helper of tests/golden/gen_mip_golden.py, never part of the build: drives the reference's own MatrixIntraPrediction members for one
// luma block.  Compiled by hand against the reference headers and linked to oracle/_ref/libvtmref.so:
//   prepareInputForPred  -> the reduced boundaries and input offsets, from a two-row buffer that holds the chosen lines (row 0: top, row 1: left, index 0 = corner)
//   predBlock            -> the prediction of one (mode, transposed)
// gen_mip_matrices copies the three trained matrices out of CommonLib/MipData.h.
#include <cstring>
#include <vector>

#include "CommonLib/Buffer.h"
#include "CommonLib/MatrixIntraPrediction.h"
#include "CommonLib/MipData.h"

extern "C" int gen_mip_case( int w, int h, int mode, int transposed, int bd, const int16_t *top, const int16_t *left, int16_t *pred )
{
  static MatrixIntraPrediction mip;
  const int stride = ( w > h ? w : h ) + 1;
  std::vector<Pel> lines( 2 * stride, 0x5555 );
  memcpy( lines.data(), top, sizeof( Pel ) * ( w + 1 ) );
  memcpy( lines.data() + stride, left, sizeof( Pel ) * ( h + 1 ) );
  const CPelBuf src( lines.data(), stride, stride, 2 );
  mip.prepareInputForPred( src, Area( 0, 0, w, h ), bd, COMPONENT_Y );
  std::vector<int> result( ( size_t ) w * h );
  mip.predBlock( result.data(), mode, transposed != 0, bd, COMPONENT_Y );
  for( int i = 0; i < w * h; i++ ) pred[i] = ( int16_t ) result[i];
  return 0;
}

extern "C" int gen_mip_matrices( uint8_t *m4x4, uint8_t *m8x8, uint8_t *m16x16 )
{
  memcpy( m4x4, mipMatrix4x4, sizeof( mipMatrix4x4 ) );
  memcpy( m8x8, mipMatrix8x8, sizeof( mipMatrix8x8 ) );
  memcpy( m16x16, mipMatrix16x16, sizeof( mipMatrix16x16 ) );
  return ( int ) ( sizeof( mipMatrix4x4 ) + sizeof( mipMatrix8x8 ) + sizeof( mipMatrix16x16 ) );
}
