// stage.hpp -- staging of the pointer-surface (host pointer) entries: every such entry copies its blocks compactly into the context's pinned staging area, uploads
// them with its job, launches a batch of one, downloads the result and copies it back to the caller's stride.  The layout of the staging area is planned by
// StagePlan (no HIP: host/test_stage.cpp runs it under sanitizers); HostStage binds a plan to the context's staging area and moves regions of it.
// The same planner at 256 bytes lays out the device workspaces of the multi-stage calls: WorkPlan binds such a plan to an arena of the context's stream.  The
// level entries read their device tables back through HostStage::pull.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

// ---- the HIP-free part -------------------------------------------------------------------------------------------
template<size_t A>
struct RegionPlan
{
  static constexpr size_t ALIGN = A;
  size_t total = 0;   // bytes planned so far (a multiple of ALIGN): the size the planned area must have
  // the next region: `bytes` long, ALIGN-aligned, behind every region handed out before (so no two overlap)
  size_t region( size_t bytes )
  {
    const size_t off = total;
    total = ( off + bytes + ALIGN - 1 ) & ~( ALIGN - 1 );
    return off;
  }
  bool inside( size_t off, size_t bytes ) const { return off <= total && bytes <= total - off; }
};
using StagePlan = RegionPlan<64>;     // the staging area of the host-pointer entries
using WorkRegions = RegionPlan<256>;  // a device workspace: an empty region takes no room, so it shares its offset with the region behind it and with nothing before it

// a w x h block of T with a row stride (in elements) <-> compact rows (stride = w)
template<class T>
inline void stage_pack( void *compact, const T *src, ptrdiff_t srcStride, int w, int h )
{
  for( int y = 0; y < h; y++ ) memcpy( ( char * ) compact + ( size_t ) y * w * sizeof( T ), src + y * srcStride, ( size_t ) w * sizeof( T ) );
}

template<class T>
inline void stage_unpack( T *dst, ptrdiff_t dstStride, const void *compact, int w, int h )
{
  for( int y = 0; y < h; y++ ) memcpy( dst + y * dstStride, ( const char * ) compact + ( size_t ) y * w * sizeof( T ), ( size_t ) w * sizeof( T ) );
}

// the offsets r * rowStep + x * stepX, r < rows, x < w, that a stepped walk over a mask / weight plane touches: lo <= 0 <= hi (its extremes are corners)
struct StageSpan
{
  long   lo = 0, hi = 0;
  size_t count() const { return ( size_t ) ( hi - lo + 1 ); }
};

inline StageSpan stage_walk_span( int w, int rows, long stepX, long rowStep )
{
  StageSpan  s;
  const long corners[3] = { ( w - 1 ) * stepX, ( rows - 1 ) * rowStep, ( rows - 1 ) * rowStep + ( w - 1 ) * stepX };
  for( long c : corners ) { s.lo = c < s.lo ? c : s.lo; s.hi = c > s.hi ? c : s.hi; }
  return s;
}

// ---- the part on top of the context (HIP translation units only) ---------------------------------------------------
#if defined( __HIPCC__ )
#include "ctx.hpp"

struct HostStage : StagePlan
{
  vtmhip_ctx *ctx;
  char       *hp = nullptr, *dp = nullptr;   // the staging area on the host (pinned) and on the device, valid after reserve()
  explicit HostStage( vtmhip_ctx *c ) : ctx( c ) {}

  // after the last region(): grows the context's staging area to the plan
  int reserve()
  {
    VTMHIP_TRY( vtmhip_internal_scratch( ctx, total ) );
    hp = ( char * ) ctx->pinned; dp = ( char * ) ctx->scratch;
    return VTMHIP_OK;
  }
  template<class T> T *host( size_t off ) const { return ( T * ) ( hp + off ); }
  template<class T> T *dev( size_t off ) const { return ( T * ) ( dp + off ); }
  template<class T> void pack( size_t off, const T *src, ptrdiff_t srcStride, int w, int h ) const { stage_pack( hp + off, src, srcStride, w, h ); }
  template<class T> void unpack( T *dst, ptrdiff_t dstStride, size_t off, int w, int h ) const { stage_unpack( dst, dstStride, hp + off, w, h ); }
  template<class J> void put( size_t off, const J &job ) const { memcpy( hp + off, &job, sizeof( J ) ); }

  // [off, off + bytes) of the staging area, host -> device / device -> host on the context's stream (off = 0: a prefix of the plan)
  int upload( size_t off, size_t bytes ) const
  {
    VTMHIP_REQUIRE( ctx, inside( off, bytes ), "staging: upload outside the planned regions" );
    VTMHIP_HIP( ctx, hipMemcpyAsync( dp + off, hp + off, bytes, hipMemcpyHostToDevice, ctx->stream ) );
    return VTMHIP_OK;
  }
  int download( size_t off, size_t bytes ) const
  {
    VTMHIP_REQUIRE( ctx, inside( off, bytes ), "staging: download outside the planned regions" );
    VTMHIP_HIP( ctx, hipMemcpyAsync( hp + off, dp + off, bytes, hipMemcpyDeviceToHost, ctx->stream ) );
    return VTMHIP_OK;
  }
  // a device table that is not the staging area's own mirror, device -> its planned region of the host side (an empty table: nothing)
  int pull( size_t off, const void *d_src, size_t bytes ) const
  {
    if( !bytes ) return VTMHIP_OK;
    VTMHIP_REQUIRE( ctx, inside( off, bytes ), "staging: pull outside the planned regions" );
    VTMHIP_HIP( ctx, hipMemcpyAsync( hp + off, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream ) );
    return VTMHIP_OK;
  }
  // behind the last download / pull of a call: the host copies are valid when this returns
  int sync() const
  {
    VTMHIP_HIP( ctx, hipStreamSynchronize( ctx->stream ) );
    return VTMHIP_OK;
  }
  int fetch( size_t off, size_t bytes ) const
  {
    VTMHIP_TRY( download( off, bytes ) );
    return sync();
  }
  // the whole read-back of a call with one job table: planned, pulled and valid on return
  template<class T> int pull_table( const T *d_src, int n, const T *&table )
  {
    const size_t off = region( ( size_t ) n * sizeof( T ) );
    VTMHIP_TRY( reserve() );
    VTMHIP_TRY( pull( off, d_src, ( size_t ) n * sizeof( T ) ) );
    table = host<T>( off );
    return sync();
  }
};

// The device workspace of a multi-stage call: regions planned at 256 bytes, bound to the arena `slot` of the context's stream by one reserve().  A layout's
// fixed head or tail (a cursor, a few small tables, slack behind the last table) is a region like the others.
struct WorkPlan : WorkRegions
{
  char *base = nullptr;   // valid after reserve()
  template<class T> size_t region( size_t count ) { return WorkRegions::region( count * sizeof( T ) ); }
  int reserve( vtmhip_ctx *ctx, vtmhip_work_slot slot )
  {
    void *arena = nullptr;
    VTMHIP_TRY( vtmhip_internal_workspace( ctx, total, &arena, slot ) );
    base = ( char * ) arena;
    return VTMHIP_OK;
  }
  template<class T> T *at( size_t off ) const { return ( T * ) ( base + off ); }
};
#endif
