// ctx.hpp -- context object and small host/device helpers shared by the libvtmhip.so translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/vtmhip.h"

// The device workspaces of one stream (vtmhip_ctx::work), every slot listed once with its owner and how long its contents must live.  Calls on one stream are
// ordered, so a slot is free again once its owner's launches are queued -- except where the note says otherwise.  Two callers that can be live at once on one
// stream must not name the same slot.
enum vtmhip_work_slot
{
  VTMHIP_WORK_CALL = 0,           // the multi-stage calls (mest.hip, pis.hip, dist.hip) and the prediction entries' shape word (intra.hip, mip.hip, intra_chroma.hip): until the call's last launch
  VTMHIP_WORK_NESTED,             // what a multi-stage call nests: the split TZ search's saved states, scan list and totals (me.hip), until its resume launch
  VTMHIP_WORK_BUCKET,             // the shape bucketing of the TU and ME chains (bucket.hpp), until its gather launch; and the AMVP SADs of the picture loop (pis.hip), which must
                                  // outlive the fused search's prologue (the search itself takes VTMHIP_WORK_CALL) -- the fused search never buckets, so the two never meet
  VTMHIP_WORK_SBT,                // the SBT chain (sbt.hip): the fused chain it runs may bucket
  VTMHIP_WORK_BOX_SUMS,           // the picture loop's 8x8 box sums (driver.hip): attached across a picture, over every call the picture makes on this stream
  VTMHIP_WORK_INTRA_CHAIN,        // the intra luma residual chain (intra_chain.hip), over the chains it runs
  VTMHIP_WORK_INTRA_CHROMA_CHAIN, // the intra chroma residual chain (intra_chroma_chain.hip), over the chains it runs
  VTMHIP_WORK_MMVD,               // the MMVD candidates' expansion (mmvd.hip): job rows, predictions and costs, over the prediction and distortion calls it runs
};

struct vtmhip_ctx
{
  int         device      = 0;
  hipStream_t ownStream   = nullptr;
  hipStream_t stream      = nullptr;   // the stream every launch goes to (own or caller-supplied)
  hipEvent_t  evStart     = nullptr;
  hipEvent_t  evStop      = nullptr;
  void       *scratch     = nullptr;   // staging area for the pointer-surface (host pointer) calls
  size_t      scratchSize = 0;
  void       *pinned      = nullptr;   // pinned host mirror of the staging area
  size_t      pinnedSize  = 0;
  // device workspaces of the multi-stage calls (vtmhip_xMotionEstimation_batch_dev ...): ONE ARENA PER STREAM the context has been pointed at, so that
  // calls queued on different streams (a level-order driver runs the levels' chains concurrently) never share scratch memory; calls on one stream are
  // ordered and reuse their arena
  struct WorkArena { void *ptr = nullptr; size_t size = 0; };
  std::map<std::pair<hipStream_t, int>, WorkArena> work;   // key: (stream, vtmhip_work_slot)
  int8_t     *lfnstTab    = nullptr;   // the caller's LFNST core matrices: g_lfnst8x8 [4][2][16][48] then g_lfnst4x4 [4][2][16][16] (vtmhip_lfnst_set_tables)
  uint8_t    *mipTab      = nullptr;   // the caller's MIP matrices: mipMatrix4x4 [16][16][4], mipMatrix8x8 [8][16][8], mipMatrix16x16 [6][64][7] (vtmhip_mip_set_tables, under initMutex)
  int32_t    *wtdFixed    = nullptr;   // DF_SSE_WTD: fixed-point luma-level weights (int64_t)( w * 65536.0 ), 1 << wtdLumaBD entries (vtmhip_set_luma_level_weights)
  int16_t    *wtdInv      = nullptr;   // DF_SSE_WTD: the reshaper's inverse LUT for VTMHIP_WTD_INV_RESHAPE_CUR jobs (valid while wtdHasInv)
  int         wtdLumaBD   = 0;         // 0: no table set yet
  int         wtdSignalType = 0;
  int32_t     wtdChromaFixed = 0;      // m_chromaWeight in the same fixed point
  bool        wtdHasInv   = false;
  int16_t    *lmcsFwd     = nullptr;   // LMCS: the reshaper's forward LUT, 1 << lmcsLumaBD entries (vtmhip_set_lmcs_fwd_lut)
  int         lmcsLumaBD  = 0;         // 0: no forward LUT set yet
  int16_t    *lmcsInv     = nullptr;   // LMCS: the reshaper's inverse LUT, 1 << lmcsInvBD entries (vtmhip_set_lmcs_inv_lut; the DF_SSE_WTD entries keep theirs in wtdInv)
  int         lmcsInvBD   = 0;         // 0: no inverse LUT set yet
  int16_t    *trTabBuf    = nullptr;   // the transform core matrices of THIS context's device (transform.hip ensure_tables; freed by vtmhip_destroy)
  const int16_t *trTab[3][7] = {};     // [type][log2 N] -> N x N forward matrix inside trTabBuf
  std::mutex  initMutex;               // guards the lazy per-context initialisations (tables, staging / workspace growth)
  int         numCUs      = 256;
  std::string lastError;
  // per-kernel launch timing (vtmhip_kernel_timing): HIP events recorded on the launch stream around every launch of the main kernels
  bool        timing      = false;
  struct TimedLaunch { const char *kernel; hipEvent_t start, stop; };
  std::vector<TimedLaunch> timed;
  std::vector<hipEvent_t>  forkEvents;   // fork / join events of vtmhip_pis_run_picture (driver.hip): created on demand, reused by every picture, freed by vtmhip_destroy
  // raster pruning (me.hip): the 8x8 box sums attached for one reference base (vtmhip_tz_attach_sums; the picture loop attaches its own per picture)
  const int16_t  *tzSumsRef   = nullptr;   // the d_refBase the sums are congruent with
  const uint16_t *tzSums      = nullptr;   // nullptr: nothing attached
  int             tzSumsW = 0, tzSumsH = 0, tzSumsMargin = 0;   // what the attached sums were computed with: a search of another picture size, or of a CTU the margin does not cover, ignores them
  hipEvent_t      tzSumsReady = nullptr;   // picture loop: recorded behind a box-sum pass that runs on a side stream; a raster launch on another stream waits for it
  hipStream_t     tzSumsJoined = nullptr;  // the stream that is already ordered behind tzSumsReady
  unsigned long long *tzStats = nullptr;   // device: scans listed, skipped, reduced, grid points evaluated, grid points total, scans accepted (vtmhip_tz_prune_stats)
  unsigned long long *tzRoundStats = nullptr;   // device: rounds bounded, candidates listed in them, candidates skipped -- first launches, then resume launches -- and violations (vtmhip_tz_round_stats)
};

// scope guard around a kernel launch: records start / stop events on ctx->stream when timing is on (bench.py's roofline: the dominant kernel's
// average launch duration, measured live on the stream the kernel is launched on)
struct vtmhip_launch_timer
{
  vtmhip_ctx *c;
  hipEvent_t  stop = nullptr;
  vtmhip_launch_timer( vtmhip_ctx *ctx, const char *kernel ) : c( ctx )
  {
    if( !c->timing ) return;
    hipEvent_t start = nullptr;
    if( hipEventCreate( &start ) != hipSuccess || hipEventCreate( &stop ) != hipSuccess ) { stop = nullptr; return; }
    ( void ) hipEventRecord( start, c->stream );
    c->timed.push_back( { kernel, start, stop } );
  }
  ~vtmhip_launch_timer() { if( stop ) ( void ) hipEventRecord( stop, c->stream ); }
};
#define VTMHIP_TIME_KERNEL( ctx, name ) vtmhip_launch_timer vtmhip_timer_guard_( ctx, name )

// every entry point starts here: a null context is an error, and the calling thread is pointed at the context's device (a host with
// several contexts / GPUs in one process, or encoder threads that never called hipSetDevice, would otherwise allocate and launch on
// whatever device happens to be current)
#define VTMHIP_CHECK_CTX( ctx )                                                                    \
  do {                                                                                             \
    if( !( ctx ) ) return VTMHIP_E_INVALID;                                                        \
    if( hipSetDevice( ( ctx )->device ) != hipSuccess )                                            \
    {                                                                                              \
      ( ctx )->lastError = "hipSetDevice failed";                                                  \
      return VTMHIP_E_HIP;                                                                         \
    }                                                                                              \
  } while( 0 )

#define VTMHIP_HIP( ctx, call )                                                                        \
  do {                                                                                                 \
    hipError_t e_ = ( call );                                                                          \
    if( e_ != hipSuccess )                                                                             \
    {                                                                                                  \
      ( ctx )->lastError = std::string( #call ) + ": " + hipGetErrorString( e_ );                      \
      return VTMHIP_E_HIP;                                                                             \
    }                                                                                                  \
  } while( 0 )

#define VTMHIP_REQUIRE( ctx, cond, msg )                   \
  do {                                                     \
    if( !( cond ) )                                        \
    {                                                      \
      ( ctx )->lastError = std::string( "invalid argument: " ) + ( msg ); \
      return VTMHIP_E_INVALID;                             \
    }                                                      \
  } while( 0 )

// launch-error check after a kernel launch (asynchronous errors surface at the next sync)
#define VTMHIP_LAUNCHED( ctx ) VTMHIP_HIP( ctx, hipGetLastError() )

// a call that returns a status: a failure is the caller's result
#define VTMHIP_TRY( call )                                 \
  do {                                                     \
    const int st_ = ( call );                              \
    if( st_ ) return st_;                                  \
  } while( 0 )

// how a _batch_dev entry starts: the context, n >= 0, nothing to do for n == 0, then the pointers the entry needs (`ptrs`: their conjunction).  An entry
// that checks something between the context and n (lmcs_resi: its LUT) writes VTMHIP_CHECK_CTX, that check, then VTMHIP_BATCH_ARGS.
#define VTMHIP_BATCH_ARGS( ctx, n, ptrs )                  \
  do {                                                     \
    VTMHIP_REQUIRE( ctx, ( n ) >= 0, "n" );                \
    if( ( n ) == 0 ) return VTMHIP_OK;                     \
    VTMHIP_REQUIRE( ctx, ptrs, "null pointer" );           \
  } while( 0 )
#define VTMHIP_BATCH_ENTRY( ctx, n, ptrs )                 \
  do {                                                     \
    VTMHIP_CHECK_CTX( ctx );                               \
    VTMHIP_BATCH_ARGS( ctx, n, ptrs );                     \
  } while( 0 )

// tuning switches of the environment; a call site keeps the value in a function-local static, so each is read once per process
inline int  env_int( const char *name, int dflt ) { const char *v = getenv( name ); return v ? atoi( v ) : dflt; }
inline bool env_switch( const char *name, bool dflt ) { return env_int( name, dflt ) != 0; }

int vtmhip_internal_scratch( vtmhip_ctx *ctx, size_t bytes );   // grows ctx->scratch / ctx->pinned
int vtmhip_internal_tr_tables( vtmhip_ctx *ctx );               // transform.hip: fills ctx->trTab / trTabBuf on first use (under initMutex)
int vtmhip_internal_tu_chain_launch( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_tu_job *d_jobs, int n, int maxWidth, int maxHeight, int uniformSize,
                                     int32_t *d_levelsBase, int16_t *d_recBase, vtmhip_tu_result *d_results );   // transform.hip: the dispatch of vtmhip_tu_chain_batch_dev
int vtmhip_internal_tu_chain_crs_launch( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_tu_job *d_jobs, int n, int maxWidth, int maxHeight, int uniformSize,
                                         int32_t *d_levelsBase, int16_t *d_recBase, vtmhip_tu_result *d_results );   // transform.hip: the dispatch of vtmhip_tu_chain_crs_batch_dev
int vtmhip_internal_jccr_chain_launch( vtmhip_ctx *ctx, bool crs, const int16_t *d_resiBase, const vtmhip_jccr_job *d_jobs, int n, int maxWidth, int maxHeight,
                                       int uniformSize, int32_t *d_levelsBase, int16_t *d_recCbBase, int16_t *d_recCrBase, vtmhip_jccr_result *d_results );   // jccr.hip: the joint chain's dispatch alone, its jobs checked by the caller
int vtmhip_internal_lfnst_expand_launch( vtmhip_ctx *ctx, const vtmhip_intra_block *d_blocks, const vtmhip_intra_job *d_intraJobs, int nIntra, const vtmhip_mip_job *d_mipJobs,
                                         const vtmhip_intra_lfnst_tu_job *d_lfnstJobs, int n, vtmhip_lfnst_chain_job *d_out, vtmhip_tu_job *d_mirror, int *d_tuBlock );   // lfnst_chain.hip
int vtmhip_internal_lfnst_chain_launch( vtmhip_ctx *ctx, const int16_t *d_resiBase, const vtmhip_lfnst_chain_job *d_jobs, int n, int maxArea, int jobInts,
                                        int32_t *d_levelsBase, int16_t *d_recBase, vtmhip_tu_result *d_results );   // lfnst_chain.hip: the LFNST chain's launch alone, its jobs checked by the caller
int vtmhip_internal_mc_launch( vtmhip_ctx *ctx, const int16_t *d_orgBase, const int16_t *d_refBase, int16_t *d_predBase, int16_t *d_outBase, const vtmhip_pred_job *d_jobs,
                               int n, int maxWidth, int maxHeight, unsigned long long *d_sadOut );   // mc.hip: motionCompensation, optionally reduced to the SAD against the original
int vtmhip_internal_mc_amvp_launch( vtmhip_ctx *ctx, const vtmhip_pic_params *pic, const int16_t *d_orgBase, const int16_t *d_refBase, const vtmhip_me_job *d_rows, int n,
                                    int maxWidth, int maxHeight, unsigned long long *d_sadOut );   // mc.hip: the AMVP candidates' predictions reduced to their SADs, jobs from the ME rows
#define VTMHIP_AFFINE_LAUNCH_WIDE 8      // `models` of vtmhip_internal_affine_me_launch: also launch the 32-bit variants (jobs with a BCW weight of -2)
int vtmhip_internal_affine_me_launch( vtmhip_ctx *ctx, const vtmhip_pic_params *pic, const int16_t *d_orgBase, const int16_t *d_refBase, const int16_t *d_otherPredBase,
                                      const vtmhip_affine_me_job *d_jobs, int n, int maxWidth, int maxHeight, vtmhip_affine_me_out *d_results, int models );   // affine.hip
struct MeFuse;      // mest_glue.hpp
int vtmhip_internal_tz_search( vtmhip_ctx *ctx, const vtmhip_pic_params *pic, const int16_t *d_orgBase, const int16_t *d_refBase, const vtmhip_tz_job *d_jobs, int n,
                               vtmhip_me_result *d_results, const MeFuse *fuse, int uniformW, int uniformH );   // me.hip: vtmhip_tz_search_batch_dev (uniformW / H != 0: every job has this shape), optionally fused with the row bookkeeping around it
struct FullFuse;    // mest_glue.hpp
int vtmhip_internal_full_search( vtmhip_ctx *ctx, const vtmhip_pic_params *pic, const int16_t *d_orgBase, const int16_t *d_refBase, const vtmhip_full_job *d_jobs, int n,
                                 int width, int height, vtmhip_me_result *d_results, const FullFuse *fuse );   // me.hip: the exhaustive searches, optionally fused
int vtmhip_internal_frac_search( vtmhip_ctx *ctx, const int16_t *d_orgBase, const int16_t *d_refBase, const vtmhip_frac_job *d_jobs, int n, int maxWidth, int maxHeight,
                                 int uniformSquare, vtmhip_frac_result *d_results, const MeFuse *fuse );   // interp.hip: vtmhip_frac_search_batch_dev, optionally fused
int vtmhip_internal_amvp_sads( vtmhip_ctx *ctx, const vtmhip_pic_params *pic, const int16_t *d_orgBase, const int16_t *d_refBase, const vtmhip_me_job *d_jobs, int n,
                               int maxWidth, int maxHeight, unsigned long long **d_dout );   // pis.hip
int vtmhip_internal_mest_with_amvp( vtmhip_ctx *ctx, const vtmhip_pic_params *pic, const vtmhip_me_cfg *cfg, const int16_t *d_orgBase, const int16_t *d_refBase,
                                    vtmhip_me_job *d_jobs, int n, int maxWidth, int maxHeight, vtmhip_me_out *d_results, const unsigned long long *d_amvpDout,
                                    unsigned long long *d_distBiP, int addIdxBits );   // mest.hip
int vtmhip_internal_mest_fusable( const vtmhip_me_cfg *cfg );
int vtmhip_internal_workspace( vtmhip_ctx *ctx, size_t bytes, void **out, vtmhip_work_slot slot = VTMHIP_WORK_CALL ); // the arena (slot) of ctx->stream, grown to `bytes` (device only); layouts: WorkPlan (stage.hpp)

// the uniform PU shapes that have tiled search kernels of their own, listed once: X( W, H ) for a shape both the exhaustive search (full_search_sq_kernel, me.hip) and
// the fractional search (frac_search_sq_kernel, interp.hip) are instantiated for, X_FRAC( W, H ) for the one only the fractional search has.  vtmhip_is_uniform_shape
// (driver.hip) answers for all of them.
#define VTMHIP_UNIFORM_SHAPES( X, X_FRAC )                                                      \
  X( 8, 8 ) X( 16, 16 ) X( 32, 32 ) X( 64, 64 ) X_FRAC( 128, 128 )                              \
  X( 16, 8 ) X( 8, 16 ) X( 32, 8 ) X( 8, 32 ) X( 32, 16 ) X( 16, 32 ) X( 64, 16 ) X( 16, 64 ) X( 64, 32 ) X( 32, 64 )
#define VTMHIP_SHAPE_NONE( W, H )

// ---- device helpers -------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_reduce_add( int v )
{
#pragma unroll
  for( int o = 32; o > 0; o >>= 1 ) v += __shfl_xor( v, o, 64 );
  return v;
}

__device__ __forceinline__ unsigned long long wave_reduce_add_u64( unsigned long long v )
{
#pragma unroll
  for( int o = 32; o > 0; o >>= 1 ) v += __shfl_xor( v, o, 64 );
  return v;
}

// wave-uniform values: tell the compiler (SGPRs, scalar branches instead of exec-mask control flow)
__device__ __forceinline__ int uni( int v ) { return __builtin_amdgcn_readfirstlane( v ); }
__device__ __forceinline__ unsigned uni( unsigned v ) { return ( unsigned ) __builtin_amdgcn_readfirstlane( ( int ) v ); }
__device__ __forceinline__ unsigned long long uni( unsigned long long v )
{
  const unsigned lo = uni( ( unsigned ) v ), hi = uni( ( unsigned ) ( v >> 32 ) );
  return ( ( unsigned long long ) hi << 32 ) | lo;
}

// XCD-aware block order: workgroups are dealt round-robin over the 8 XCDs (blocks b and b + 8 share an L2), so block b takes
// the work item at position (b % 8) * (n / 8) + b / 8 (bijective for any n): the workgroups running on one XCD at any moment
// then hold NEIGHBOURING jobs of the table (PUs in raster order), whose search windows overlap and stay in that XCD's 4 MiB L2.
__device__ __forceinline__ int xcd_order( int b, int n )
{
  const int q = n >> 3, r = n & 7, xcd = b & 7;
  return ( xcd < r ? xcd * ( q + 1 ) : r * ( q + 1 ) + ( xcd - r ) * q ) + ( b >> 3 );
}
