// ciip_host.hpp -- combined inter-intra prediction of one job as host arithmetic, without a HIP dependency: the bodies of vtmhip_ciip_host and
// vtmhip_ciip_blend_host (ciip.hip), which host/test_ciip.cpp compiles with g++ under the sanitizers.  The rules are ciip_rules.hpp's, the Hadamard tile of a block
// had_tile_rule.hpp's; the tile itself is evaluated in 32 bits as had_finish (had.hpp) evaluates it on the device.
#pragma once
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ciip_rules.hpp"
#include "had_tile_rule.hpp"

namespace
{

constexpr uint64_t CIIP_HOST_NO_COST = ~( uint64_t ) 0;

inline uint64_t ciipHostHadTile( HadTile t, const int16_t *o, int os, const int16_t *c, int cs )
{
  int m[128];
  for( int y = 0; y < t.h; y++ )
    for( int x = 0; x < t.w; x++ ) m[y * t.w + x] = ( int ) o[y * os + x] - ( int ) c[y * cs + x];
  for( int pass = 0; pass < 2; pass++ )   // rows, then columns
  {
    const int len = pass ? t.h : t.w, cnt = pass ? t.w : t.h, step = pass ? t.w : 1, next = pass ? 1 : t.w;
    for( int r = 0; r < cnt; r++ )
      for( int s = 1; s < len; s <<= 1 )
        for( int i = 0; i < len; i += s << 1 )
          for( int k = i; k < i + s; k++ )
          {
            const int a = m[r * next + k * step], b = m[r * next + ( k + s ) * step];
            m[r * next + k * step] = a + b; m[r * next + ( k + s ) * step] = a - b;
          }
  }
  int sum = 0;
  for( int i = 0; i < t.w * t.h; i++ ) sum += abs( m[i] );
  const int dc = abs( m[0] );
  sum = sum - dc + ( dc >> 2 );
  if( t.w == 2 ) return ( uint64_t ) sum;
  if( t.w == 4 && t.h == 4 ) return ( uint64_t ) ( ( sum + 1 ) >> 1 );
  if( t.w == 8 && t.h == 8 ) return ( uint64_t ) ( ( sum + 2 ) >> 2 );
  if( t.w * t.h == 128 ) return ( uint64_t ) ( int ) ( ( double ) sum / 11.313708498984761 * 2.0 );   // sqrt(16.0*8)
  return ( uint64_t ) ( int ) ( ( double ) sum / 5.656854249492381 * 2.0 );                          // sqrt(4.0*8)
}

// cur: w x h, stride w
inline void ciipHostCosts( const int16_t *org, int os, const int16_t *cur, int w, int h, uint64_t &satd, uint64_t &sad )
{
  const HadTile t = had_tile_shape( w, h );
  satd = sad = 0;
  for( int y = 0; y < h; y += t.h )
    for( int x = 0; x < w; x += t.w ) satd += ciipHostHadTile( t, org + y * os + x, os, cur + y * w + x, w );
  for( int y = 0; y < h; y++ )
    for( int x = 0; x < w; x++ ) sad += ( uint64_t ) abs( ( int ) org[y * os + x] - ( int ) cur[y * w + x] );
}

// 0, or -1 for a job the table predicate rejects or a missing pointer: nothing is written then
inline int ciipHostJob( const vtmhip_ciip_job *job, const int16_t *lineBase, const int16_t *orgBase, const int16_t *const inter[VTMHIP_CIIP_MAX_CAND], const int16_t *fwdLut,
                        const int16_t *invLut, int16_t *blend, uint64_t satd[VTMHIP_CIIP_MAX_CAND], uint64_t sad[VTMHIP_CIIP_MAX_CAND] )
{
  if( !job || !lineBase || !orgBase || !inter || !blend || !satd || !sad ) return -1;
  if( !ciipJobOk( *job, 64, 64, fwdLut && invLut ? job->bitDepth : 0 ) ) return -1;
  for( int k = 0; k < job->numCand; k++ )
    if( !inter[k] ) return -1;
  const int            w = job->width, h = job->height, bd = job->bitDepth, wIntra = ciipWeightIntra( job->leftIntra, job->aboveIntra );
  std::vector<int16_t> intra( ( size_t ) w * h ), cur( ( size_t ) w * h );
  ciipHostIntra( lineBase + job->lineOff, w, h, bd, false, intra.data() );
  for( int k = 0; k < VTMHIP_CIIP_MAX_CAND; k++ )
  {
    satd[k] = sad[k] = CIIP_HOST_NO_COST;
    if( k >= job->numCand ) continue;
    int16_t *dst = blend + ( size_t ) k * w * h;
    memcpy( dst, inter[k], sizeof( int16_t ) * w * h );
    ciipHostBlend( dst, w, intra.data(), w, h, bd, wIntra, job->lmcs ? fwdLut : nullptr );
    for( int i = 0; i < w * h; i++ ) cur[i] = job->lmcs ? ( int16_t ) ciipLutAt( invLut, dst[i], ( 1 << bd ) - 1 ) : dst[i];
    ciipHostCosts( orgBase + job->orgOff, job->orgStride, cur.data(), w, h, satd[k], sad[k] );
  }
  return 0;
}

inline int ciipHostBlendJob( const vtmhip_ciip_blend_job *job, const int16_t *lineBase, int16_t *predBase, const int16_t *fwdLut )
{
  if( !job || !lineBase || !predBase || !ciipBlendJobOk( *job, fwdLut ? job->bitDepth : 0 ) ) return -1;
  std::vector<int16_t> intra( ( size_t ) job->width * job->height );
  ciipHostIntra( lineBase + job->lineOff, job->width, job->height, job->bitDepth, job->chroma != 0, intra.data() );
  ciipHostBlend( predBase + job->predOff, job->predStride, intra.data(), job->width, job->height, job->bitDepth, ciipWeightIntra( job->leftIntra, job->aboveIntra ),
                 job->mapFwd ? fwdLut : nullptr );
  return 0;
}

}   // namespace
