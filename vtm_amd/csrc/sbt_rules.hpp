// sbt_rules.hpp -- the sub-block transform (SBT) rules of the reference, defined once for host and device: plain integer (and, for the RD-cost skip, double)
// functions without a HIP dependency, so host/test_sbt.cpp compiles them with g++ and the kernels of sbt.hip use the same text.
//   sbtAllowed              CodingUnit::checkAllowedSbt, the size part                    CommonLib/Unit.cpp:450-494
//   getSbtMode ...          CU::getSbtMode / getSbtIdxFromSbtMode / getSbtPosFromSbtMode / targetSbtAllowed / numSbtModeRdo
//                                                                                         CommonLib/UnitTools.cpp:3516-3589
//   sbtCodedTile            PartitionerImpl::getSbtTuTiling, the tile that carries the residual   CommonLib/UnitPartitioner.cpp:1091-1148
//   sbtTrTypes              TrQuant::getTrTypes, the isSBT branch (luma; chroma is DCT-2)  CommonLib/TrQuant.cpp:728-760
//   sbtNumPart              the partition count of InterSearch::calcMinDistSbt            EncoderLib/InterSearch.cpp:6214-6215
//   sbtCombine              calcMinDistSbt from the 4 x 4 partition distortions on        :6261-6386
//   sbtSkipByRdCost         InterSearch::skipSbtByRDCost                                  :6389-6438
#pragma once
#include <stdint.h>

#if defined( __HIPCC__ )
#define SBT_HD __host__ __device__ inline
#else
#define SBT_HD inline
#endif

enum { SBT_OFF_DCT = 0, SBT_VER_HALF = 1, SBT_HOR_HALF = 2, SBT_VER_QUAD = 3, SBT_HOR_QUAD = 4, NUMBER_SBT_IDX = 5 };
enum { SBT_POS0 = 0, SBT_POS1 = 1 };
enum { SBT_VER_H0 = 0, SBT_VER_H1, SBT_HOR_H0, SBT_HOR_H1, SBT_VER_Q0, SBT_VER_Q1, SBT_HOR_Q0, SBT_HOR_Q1, NUMBER_SBT_MODE };
enum { SBT_NUM_RDO = 2, SBT_TR_DCT2 = 0, SBT_TR_DCT8 = 1, SBT_TR_DST7 = 2, SBT_MTS_INTER_MAX_CU_SIZE = 32 };

// bit i set: sbtIdx i may be used.  The prediction-mode / CIIP / SPS conditions of checkAllowedSbt stay the caller's.
SBT_HD int sbtAllowed( int cuW, int cuH, int maxTbSize )
{
  const int minSbtCUSize = 8;   // 1 << ( MIN_CU_LOG2 + 1 )
  if( cuW > maxTbSize || cuH > maxTbSize ) return 0;
  return ( ( cuW >= minSbtCUSize ) << SBT_VER_HALF ) | ( ( cuH >= minSbtCUSize ) << SBT_HOR_HALF ) | ( ( cuW >= 2 * minSbtCUSize ) << SBT_VER_QUAD ) |
         ( ( cuH >= 2 * minSbtCUSize ) << SBT_HOR_QUAD );
}

SBT_HD int getSbtMode( int sbtIdx, int sbtPos ) { return ( sbtIdx - SBT_VER_HALF ) * 2 + sbtPos; }
SBT_HD int getSbtIdxFromSbtMode( int sbtMode ) { return sbtMode <= SBT_VER_H1 ? SBT_VER_HALF : sbtMode <= SBT_HOR_H1 ? SBT_HOR_HALF : sbtMode <= SBT_VER_Q1 ? SBT_VER_QUAD : SBT_HOR_QUAD; }
SBT_HD int getSbtPosFromSbtMode( int sbtMode ) { return sbtMode & 1; }
SBT_HD int targetSbtAllowed( int sbtIdx, int allowed ) { return sbtIdx >= SBT_VER_HALF && sbtIdx <= SBT_HOR_QUAD ? ( allowed >> sbtIdx ) & 1 : 0; }
SBT_HD int numSbtModeRdo( int allowed )
{
  const int half = targetSbtAllowed( SBT_VER_HALF, allowed ) + targetSbtAllowed( SBT_HOR_HALF, allowed );
  const int quad = targetSbtAllowed( SBT_VER_QUAD, allowed ) + targetSbtAllowed( SBT_HOR_QUAD, allowed );
  return ( 2 * half < SBT_NUM_RDO ? 2 * half : SBT_NUM_RDO ) + ( 2 * quad < SBT_NUM_RDO ? 2 * quad : SBT_NUM_RDO );
}

// The coded tile of a component block cw x ch: offsets and sizes are (dim * factor) >> 2 on the component's own block.  POS0 codes tile 0 (offset 0, 1/2 or 1/4 of
// the side), POS1 tile 1 (offset 1/2 or 3/4); the other tile of the pair carries no residual.
SBT_HD void sbtCodedTile( int cw, int ch, int sbtIdx, int sbtPos, int &x, int &y, int &w, int &h )
{
  const bool quad = sbtIdx >= SBT_VER_QUAD, hor = sbtIdx == SBT_HOR_HALF || sbtIdx == SBT_HOR_QUAD;
  const int  sizeFactor = quad ? 1 : 2, offFactor = sbtPos == SBT_POS0 ? 0 : 4 - sizeFactor;
  x = hor ? 0 : ( cw * offFactor ) >> 2;
  y = hor ? ( ch * offFactor ) >> 2 : 0;
  w = hor ? cw : ( cw * sizeFactor ) >> 2;
  h = hor ? ( ch * sizeFactor ) >> 2 : ch;
}

// the transform pair of the LUMA sub-TU tuW x tuH (no transform skip and no MTS on an SBT CU: TU::isTSAllowed, UnitTools.cpp:3819)
SBT_HD void sbtTrTypes( int sbtIdx, int sbtPos, int tuW, int tuH, int &trHor, int &trVer )
{
  if( sbtIdx == SBT_VER_HALF || sbtIdx == SBT_VER_QUAD )
  {
    if( tuH > SBT_MTS_INTER_MAX_CU_SIZE ) { trHor = trVer = SBT_TR_DCT2; return; }
    trHor = sbtPos == SBT_POS0 ? SBT_TR_DCT8 : SBT_TR_DST7;
    trVer = SBT_TR_DST7;
  }
  else
  {
    if( tuW > SBT_MTS_INTER_MAX_CU_SIZE ) { trHor = trVer = SBT_TR_DCT2; return; }
    trHor = SBT_TR_DST7;
    trVer = sbtPos == SBT_POS0 ? SBT_TR_DCT8 : SBT_TR_DST7;
  }
}

// The right shift of a squared sample difference.  calcMinDistSbt (:6229) takes DISTORTION_PRECISION_ADJUSTMENT( ( bitDepth - 8 ) << 1 ), RdCost::xGetSSE (the
// uncoded tile, the chain's SSE) DISTORTION_PRECISION_ADJUSTMENT( bitDepth ) << 1.  The reference is built with FULL_NBIT = 1 (TypeDef.h:228-233), which makes
// the macro 0 for every argument: both shifts are 0 and distortions keep all bits.  (With FULL_NBIT = 0 the macro is max( x - 8, 0 ): xGetSSE would shift by
// ( bitDepth - 8 ) * 2, calcMinDistSbt -- whose argument is at most 8 up to 12 bits -- still by 0.)  Without a shift a 16 x 16 partition at 12 bits reaches
// 256 * 4095^2 = 4 292 870 400, 2 096 896 below 2^32: the 32-bit partition sums rest on samples inside the bit depth (|org - pred| <= 4095).
SBT_HD int sbtDistShift( int /* bitDepth */ ) { return 0; }

SBT_HD int sbtNumPart( int lumaSide ) { return lumaSide >= 16 ? 4 : lumaSide == 4 ? 1 : 2; }

// calcMinDistSbt after the sample pass.  dist[j][i]: the partition distortions (luma + weighted chroma), zero outside numPartY x numPartX.  Fills est[9]
// (est[8] = the CU's SSE; modes that are not tried stay at UINT64_MAX) and rdoOrder[8] (255-filled); returns skipAll.  On skipAll the mode estimates and the order
// stay untouched, as in the reference's early return.
SBT_HD int sbtCombine( const uint64_t dist[4][4], int numPartX, int numPartY, int allowed, double distScale, uint64_t est[9], uint8_t rdoOrder[8] )
{
  const uint64_t maxDist = ~( uint64_t ) 0;
  est[NUMBER_SBT_MODE] = 0;
  for( int j = 0; j < 4; j++ )
    for( int i = 0; i < 4; i++ )
      if( j < numPartY && i < numPartX ) est[NUMBER_SBT_MODE] += dist[j][i];
  for( int m = 0; m < NUMBER_SBT_MODE; m++ ) { est[m] = maxDist; rdoOrder[m] = 255; }
  // SBT fast algorithm 1: calcRdCost( 0, dist ) < calcRdCost( 12 << SCALE_BITS, 0 )
  if( distScale * double( est[NUMBER_SBT_MODE] ) + 0.0 < distScale * 0.0 + double( ( uint64_t ) 12 << 15 ) ) return 1;

  const int shift = 5;
  if( targetSbtAllowed( SBT_VER_HALF, allowed ) )
  {
    uint64_t resi = 0, noResi = 0;
    for( int j = 0; j < 4; j++ )
      for( int i = 0; i < 2; i++ )
        if( j < numPartY && i < numPartX / 2 ) { resi += dist[j][i]; noResi += dist[j][i + numPartX / 2]; }
    est[SBT_VER_H0] = ( resi >> shift ) + noResi;
    est[SBT_VER_H1] = ( noResi >> shift ) + resi;
  }
  if( targetSbtAllowed( SBT_HOR_HALF, allowed ) )
  {
    uint64_t resi = 0, noResi = 0;
    for( int j = 0; j < 2; j++ )
      for( int i = 0; i < 4; i++ )
        if( j < numPartY / 2 && i < numPartX ) { resi += dist[j][i]; noResi += dist[j + numPartY / 2][i]; }
    est[SBT_HOR_H0] = ( resi >> shift ) + noResi;
    est[SBT_HOR_H1] = ( noResi >> shift ) + resi;
  }
  if( targetSbtAllowed( SBT_VER_QUAD, allowed ) )   // numPartX == 4
  {
    uint64_t q0 = 0, q1 = 0;
    for( int j = 0; j < 4; j++ )
      if( j < numPartY )
      {
        q0 += dist[j][0] + ( ( dist[j][1] + dist[j][2] + dist[j][3] ) << shift );
        q1 += dist[j][3] + ( ( dist[j][0] + dist[j][1] + dist[j][2] ) << shift );
      }
    est[SBT_VER_Q0] = q0 >> shift;
    est[SBT_VER_Q1] = q1 >> shift;
  }
  if( targetSbtAllowed( SBT_HOR_QUAD, allowed ) )   // numPartY == 4
  {
    uint64_t q0 = 0, q1 = 0;
    for( int i = 0; i < 4; i++ )
      if( i < numPartX )
      {
        q0 += dist[0][i] + ( ( dist[1][i] + dist[2][i] + dist[3][i] ) << shift );
        q1 += dist[3][i] + ( ( dist[0][i] + dist[1][i] + dist[2][i] ) << shift );
      }
    est[SBT_HOR_Q0] = q0 >> shift;
    est[SBT_HOR_Q1] = q1 >> shift;
  }

  // SBT fast algorithm 5: the modes with the lowest estimate first, half modes then quad modes; strict `<`, so a tie goes to the lower mode
  uint64_t temp[NUMBER_SBT_MODE];
  for( int m = 0; m < NUMBER_SBT_MODE; m++ ) temp[m] = est[m];
  uint64_t order = ~( uint64_t ) 0;   // the eight order bytes, entry `pos` in bits 8 pos .. 8 pos + 7 (no indexed local array on the device)
  int      pos   = 0;
  for( int cls = 0; cls < 2; cls++ )
  {
    const int first = cls ? SBT_VER_Q0 : SBT_VER_H0;
    int       num   = targetSbtAllowed( cls ? SBT_VER_QUAD : SBT_VER_HALF, allowed ) + targetSbtAllowed( cls ? SBT_HOR_QUAD : SBT_HOR_HALF, allowed );
    num = 2 * num < SBT_NUM_RDO ? 2 * num : SBT_NUM_RDO;
    for( int k = 0; k < SBT_NUM_RDO; k++ )
    {
      if( k >= num ) continue;
      uint64_t minDist = maxDist;
      int      best    = 255;
      for( int m = first; m < first + 4; m++ )
        if( temp[m] < minDist ) { minDist = temp[m]; best = m; }
      order = ( order & ~( ( uint64_t ) 255 << ( 8 * pos ) ) ) | ( ( uint64_t ) best << ( 8 * pos ) );
      pos++;
      for( int m = first; m < first + 4; m++ )   // an allowed mode's estimate is below UINT64_MAX, so `best` is a mode here
        if( m == best ) temp[m] = maxDist;
    }
  }
  for( int m = 0; m < NUMBER_SBT_MODE; m++ ) rdoOrder[m] = ( uint8_t ) ( order >> ( 8 * m ) );
  return 0;
}

// InterSearch::skipSbtByRDCost over an est[9] record: 0 .. 3 = the early-skip type, 255 = try the mode.  The double operations are the reference's, in its order
// (calcRdCost( bits, dist ) = distScale * double( dist ) + double( bits ); MAX_DOUBLE = 1.7e+308).
SBT_HD int sbtSkipByRdCost( const uint64_t est[9], double distScale, int sbtIdx, int sbtPos, double bestCost, uint64_t distSbtOff, double costSbtOff, int rootCbfSbtOff )
{
  const int      sbtMode = getSbtMode( sbtIdx, sbtPos );
  const uint64_t scale11 = ( uint64_t ) 11 << 15, scale10 = ( uint64_t ) 10 << 15;
  if( distScale * double( est[sbtMode] ) + double( scale11 ) > bestCost ) return 0;
  if( costSbtOff != 1.7e+308 )
  {
    if( !rootCbfSbtOff )
    {
      uint64_t distResiPart;
      if( sbtIdx == SBT_VER_HALF || sbtIdx == SBT_HOR_HALF ) distResiPart = ( ( est[NUMBER_SBT_MODE] - est[sbtMode] ) * 9 ) >> 4;
      else distResiPart = ( ( est[NUMBER_SBT_MODE] - est[sbtMode] ) * 3 ) >> 3;
      const double estCost = ( costSbtOff - ( distScale * double( distSbtOff ) + double( ( uint64_t ) 0 ) ) ) + ( distScale * double( est[sbtMode] + distResiPart ) + double( scale10 ) );
      if( estCost > costSbtOff ) return 1;
      if( estCost > bestCost ) return 2;
    }
    else
    {
      const double weight  = sbtMode > SBT_HOR_H1 ? 0.4 : 0.6;
      const double estCost = ( ( costSbtOff - ( distScale * double( distSbtOff ) + double( ( uint64_t ) 0 ) ) ) * weight ) + ( distScale * double( est[sbtMode] ) + double( ( uint64_t ) 0 ) );
      if( estCost > bestCost ) return 3;
    }
  }
  return 255;
}
