// pel_pack.hpp -- several consecutive 16-bit samples as one memory access, and their unpacking to / packing from one int per sample (device code only).
#pragma once
#include <cstdint>

// 2 / 4 / 8 samples at a 2-byte aligned address: one 4- / 8- / 16-byte access (gfx950 global memory handles the misalignment in hardware: it splits the access
// only when the address asks for it); Dw2 / Dw4: the same dwords at a 4-byte aligned address
struct __attribute__( ( packed, aligned( 2 ) ) ) Pel2 { unsigned v; };
struct __attribute__( ( packed, aligned( 2 ) ) ) Pel4 { unsigned v[2]; };
struct __attribute__( ( packed, aligned( 2 ) ) ) Pel8 { unsigned v[4]; };
struct __attribute__( ( packed, aligned( 4 ) ) ) Dw2 { unsigned v[2]; };
struct __attribute__( ( packed, aligned( 4 ) ) ) Dw4 { unsigned v[4]; };

__device__ __forceinline__ void unpack4( const Pel4 t, int a[4] )
{
#pragma unroll
  for( int k = 0; k < 2; k++ ) { a[2 * k] = ( int ) ( short ) ( t.v[k] & 0xffffu ); a[2 * k + 1] = ( int ) t.v[k] >> 16; }
}
__device__ __forceinline__ void unpack8( const unsigned u[4], int a[8] )
{
#pragma unroll
  for( int k = 0; k < 4; k++ ) { a[2 * k] = ( int ) ( short ) ( u[k] & 0xffffu ); a[2 * k + 1] = ( int ) u[k] >> 16; }
}
__device__ __forceinline__ void unpack8( const Pel8 t, int a[8] ) { unpack8( t.v, a ); }
__device__ __forceinline__ Pel4 pack4( const int v[4] )   // the low 16 bits of every value (Pel wrap)
{
  Pel4 t;
  t.v[0] = ( ( unsigned ) v[0] & 0xffffu ) | ( ( unsigned ) v[1] << 16 ); t.v[1] = ( ( unsigned ) v[2] & 0xffffu ) | ( ( unsigned ) v[3] << 16 );
  return t;
}

// the first cnt (1..4) samples of a 4-sample row segment: a whole segment moves as one 8-byte access, a ragged one sample by sample (v[k] = 0 for k >= cnt)
__device__ __forceinline__ void ld4( const int16_t *p, int cnt, int v[4] )
{
  if( cnt == 4 ) unpack4( *reinterpret_cast<const Pel4 *>( p ), v );
  else
  {
#pragma unroll
    for( int k = 0; k < 4; k++ ) v[k] = k < cnt ? p[k] : 0;
  }
}
__device__ __forceinline__ void st4( int16_t *p, int cnt, const int v[4] )
{
  if( cnt == 4 ) *reinterpret_cast<Pel4 *>( p ) = pack4( v );
  else
  {
#pragma unroll
    for( int k = 0; k < 4; k++ )
      if( k < cnt ) p[k] = ( int16_t ) v[k];
  }
}
