// had_tile_rule.hpp -- the rule that picks the Hadamard tile of a W x H block (xGetHADs, RdCost.cpp:2837-2931), stated here and nowhere else: had.hpp evaluates the
// tile it names on the device, dist.hip counts tiles with it on the host, ciip_host.hpp walks them on the host.  No HIP dependency.
#pragma once

#if defined( __HIPCC__ )
#define HAD_RULE_HD __host__ __device__ constexpr
#else
#define HAD_RULE_HD constexpr
#endif

namespace
{

// ---- the tile that xGetHADs cuts a W x H block into (RdCost.cpp:2837-2931): the one statement of the rule, host and device -------------------
struct HadTile { int w, h; };

HAD_RULE_HD HadTile had_tile_shape( int w, int h )
{
  if( w > h && ( h & 7 ) == 0 && ( w & 15 ) == 0 ) return { 16, 8 };
  if( w < h && ( w & 7 ) == 0 && ( h & 15 ) == 0 ) return { 8, 16 };
  if( w > h && ( h & 3 ) == 0 && ( w & 7 ) == 0 ) return { 8, 4 };
  if( w < h && ( w & 3 ) == 0 && ( h & 7 ) == 0 ) return { 4, 8 };
  if( ( h & 7 ) == 0 && ( w & 7 ) == 0 ) return { 8, 8 };
  if( ( h & 3 ) == 0 && ( w & 3 ) == 0 ) return { 4, 4 };
  return { 2, 2 };
}

constexpr bool had_tile_is( int w, int h, int tw, int th ) { return had_tile_shape( w, h ).w == tw && had_tile_shape( w, h ).h == th; }
// one shape per branch, and the shapes at which a rule narrowed to powers of two, or to sides from 8, answers differently
static_assert( had_tile_is( 32, 8, 16, 8 ) && had_tile_is( 8, 32, 8, 16 ), "xGetHADs: 16x8 / 8x16" );
static_assert( had_tile_is( 24, 8, 8, 4 ) && had_tile_is( 16, 4, 8, 4 ), "xGetHADs: 8x4 (24 is no multiple of 16)" );
static_assert( had_tile_is( 8, 24, 4, 8 ) && had_tile_is( 12, 16, 4, 8 ), "xGetHADs: 4x8" );
static_assert( had_tile_is( 8, 8, 8, 8 ), "xGetHADs: 8x8" );
static_assert( had_tile_is( 12, 12, 4, 4 ) && had_tile_is( 4, 4, 4, 4 ), "xGetHADs: 4x4" );
static_assert( had_tile_is( 6, 4, 2, 2 ) && had_tile_is( 2, 2, 2, 2 ), "xGetHADs: 2x2" );

}   // namespace
