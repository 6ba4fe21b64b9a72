// isp_chain.hip -- intra sub-partitions (ISP) on the device: one (CU, intra mode, split direction) candidate per job, every sub-partition of it in one kernel; the
// rules are isp_rules.hpp's, the quant rule, the passes, the group synchronisation and the reduction tu_stages.hpp's.
//   vtmhip_isp_chain_batch_dev   per sub-partition the steps of IntraSearch::xIntraCodingTUBlock with cu.ispMode set: the prediction of its region from the
//                                reconstruction of the one before, residual, xT -> quant -> dequant -> xIT, clipped reconstruction, SSE   (EncoderLib/IntraSearch.cpp:2989-3320,
//                                CommonLib/IntraPrediction.cpp:802-918)
//   vtmhip_isp_chain_host        the same as host arithmetic (isp_host.hpp)
//   vtmhip_isp_geometry / _pred_params / _tr_types / _pred_region_host / _next_lines_host   the single rules on the host
//
// isp_chain_kernel<LANES>: a job gets LANES lanes (16: sixteen jobs per workgroup, 64: a wave per job, 256: the workgroup); groups of up to 64 lanes lie inside a wave
// and meet at chain_sync, only the 256-lane form uses workgroup barriers.  Per job in LDS (IspPlan, sized by the host from the table): two int blocks of one TU (the
// residual / coefficients and the block between two passes), the original and the reconstruction so far as int16, the CU's two lines and the two a later region
// sees, and the two core matrices of the TU shape -- the sub-partitions of a CU share one shape -- transposed for the forward passes and plain for the inverse
// ones.  The walk: per prediction region its lines (region 0: the CU's; later ones: ispMainAt / ispSideAt over the CU's lines and the reconstruction in LDS, written
// out once per region), its prediction, stored where the reconstruction will lie; per TU of the region the residual against the staged original, the passes, the
// quantiser in place, the inverse passes with the clipped reconstruction as their epilogue, and the three sums of the TU.  Nothing of a candidate touches global memory
// between the first loads and the stores of the prediction, the levels, the results and the finished reconstruction.  A group past the end of the table repeats the
// last job in its own slot and stores nothing.  The entry reads both tables back through HostStage (stage.hpp) and checks them before anything runs.
#include "ctx.hpp"
#include "stage.hpp"
#include "tu_stages.hpp"
#include "chroma_taps.hpp"
#include "intra_lane_rule.hpp"
#include "isp_rules.hpp"
#include "isp_host.hpp"

namespace
{

__constant__ int16_t c_ispCubic[32][4] = { VTMHIP_CHROMA_FILTER_TAPS };   // InterpolationFilter::getChromaFilterTable (IntraPrediction.cpp:576)

struct IspTabs { const int16_t *m[2][7]; };   // [0: DCT2, 1: DST7][log2 N] -> the N x N forward matrix (row-major), the context's

template<int LANES>
__global__ __launch_bounds__( 256 ) void isp_chain_kernel( const int16_t *__restrict__ refBase, const int16_t *__restrict__ orgBase, const vtmhip_intra_block *__restrict__ blocks,
                                                          const vtmhip_isp_job *__restrict__ jobs, int numJobs, IspTabs tabs, IspPlan plan, int16_t *__restrict__ predBase,
                                                          int *__restrict__ levelsBase, int16_t *__restrict__ recoBase, vtmhip_isp_result *__restrict__ results )
{
  extern __shared__ __attribute__( ( aligned( 16 ) ) ) int ldsw[];
  __shared__ long long sRed[4][3];
  constexpr int G = 256 / LANES;
  const int  sub = threadIdx.x / LANES, t = threadIdx.x % LANES, jobIdx = blockIdx.x * G + sub;
  const bool live = jobIdx < numJobs;
  const vtmhip_isp_job     J = jobs[live ? jobIdx : numJobs - 1];
  const vtmhip_intra_block B = blocks[J.block];
  const int W = B.width, H = B.height, bd = B.bitDepth, maxVal = ( 1 << bd ) - 1, lW = intraLog2( W ), split = J.split, mode = J.mode;
  IspGeom   g;
  ispGeometry( W, H, split, g );
  const int pw = g.partW, ph = g.partH, lpw = intraLog2( pw ), lph = intraLog2( ph ), lrw = intraLog2( g.regW ), partArea = pw * ph;
  const int skipW = ispTrSkip( pw ), skipH = ispTrSkip( ph );

  int     *bufA  = ldsw + sub * plan.jobInts, *bufB = bufA + plan.partArea;
  int16_t *sOrg  = ( int16_t * ) ( bufB + plan.partArea ), *sReco = sOrg + plan.maxArea;
  int16_t *sTop  = sReco + plan.maxArea, *sLeft = sTop + plan.line, *sMain = sLeft + plan.line, *sSide = sMain + plan.line;
  int16_t *sMwT  = sSide + plan.line, *sMw = sMwT + ( pw > 1 ? pw * pw : 0 ), *sMhT = sMw + ( pw > 1 ? pw * pw : 0 ), *sMh = sMhT + ( ph > 1 ? ph * ph : 0 );

  {
    const int16_t *ref = refBase + B.refOff, *org = orgBase + B.orgOff;
    for( int i = t; i < 2 * W + 1; i += LANES ) sTop[i] = ref[i];
    for( int i = t; i < 2 * H + 1; i += LANES ) sLeft[i] = ref[2 * W + 1 + i];
    for( int i = t; i < W * H; i += LANES ) sOrg[i] = org[( long ) ( i >> lW ) * B.orgStride + ( i & ( W - 1 ) )];
    if( pw > 1 )
    {
      const int16_t *m = tabs.m[ispTrType( pw ) == VTMHIP_DST7][lpw];
      lds_load_matrix_T( m, pw, sMwT, t, LANES );
      lds_load_matrix( m, pw, sMw, t, LANES );
    }
    if( ph > 1 )
    {
      const int16_t *m = tabs.m[ispTrType( ph ) == VTMHIP_DST7][lph];
      lds_load_matrix_T( m, ph, sMhT, t, LANES );
      lds_load_matrix( m, ph, sMh, t, LANES );
    }
  }
  chain_sync<LANES>();

  const QuantRule   qr  = quant_rule( bd, J.qpPer, J.qpRem, J.isIRAP, lpw, lph, false );
  vtmhip_isp_result *res = results + ( live ? jobIdx : 0 );
  int16_t           *pred = ( predBase && live ) ? predBase + J.predOff : nullptr;
  int               *levels = ( levelsBase && live ) ? levelsBase + J.outOff : nullptr;
  vtmhip_intra_params p;
  ispPredParams( W, H, g.regW, g.regH, mode, p );

  for( int r = 0; r < g.numRegions; r++ )
  {
    const int rx = split == ISP_HOR ? 0 : r * g.ext, ry = split == ISP_HOR ? r * g.ext : 0;
    IspBlk    b;
    b.w = g.regW; b.h = g.regH; b.log2W = lrw; b.log2H = intraLog2( g.regH ); b.m = 0; b.maxVal = maxVal;
    b.topLast = W + g.regW; b.leftLast = H + g.regH;
    if( r == 0 ) { b.top = sTop; b.left = sLeft; }
    else
    {
      const IspLines lines = { sTop, sLeft, sReco, W, split, J.sideAvail };
      const int      mainLast = split == ISP_HOR ? b.topLast : b.leftLast, sideLast = split == ISP_HOR ? b.leftLast : b.topLast;
      for( int i = t; i <= mainLast; i += LANES ) sMain[i] = ( int16_t ) ispMainAt( lines, g, r, i );
      for( int i = t; i <= sideLast; i += LANES ) sSide[i] = ( int16_t ) ispSideAt( lines, g, r, i );
      b.top = split == ISP_HOR ? sMain : sSide; b.left = split == ISP_HOR ? sSide : sMain;
      chain_sync<LANES>();
    }
    const int dcVal = mode == INTRA_DC ? intraDcVal( b ) : 0;
    for( int i = t; i < g.regW * g.regH; i += LANES )
    {
      const int     x = i & ( g.regW - 1 ), y = i >> lrw, at = ( ry + y ) * W + rx + x;
      const int16_t v = intraPredSample( p, mode, b, dcVal, c_ispCubic, x, y );
      sReco[at] = v;   // the prediction lies where the reconstruction will
      if( pred ) pred[at] = v;
    }
    chain_sync<LANES>();

    for( int q = 0; q < g.tusPerRegion; q++ )
    {
      const int k = r * g.tusPerRegion + q;
      int       px, py;
      ispPartRect( g, split, k, px, py );
      for( int i = t; i < partArea; i += LANES )
      {
        const int at = ( py + ( i >> lpw ) ) * W + px + ( i & ( pw - 1 ) );
        bufA[i] = ( int ) sOrg[at] - ( int ) sReco[at];
      }
      chain_sync<LANES>();
      long long sumAbs = 0, absSum = 0, sse = 0;
      int      *coef;
      // TrQuant::xT: rows with the horizontal matrix, then columns with the vertical one; the one pass of a TU with a side of 1
      if( pw > 1 && ph > 1 )
      {
        lds_fwd_pass( bufA, pw, bufB, ph, sMwT, pw, ph, ALL_LINES, pw - skipW, ispFwdShift1( lpw, bd ), t, LANES, ( long long * ) nullptr );
        chain_sync<LANES>();
        lds_fwd_pass( bufB, ph, bufA, pw, sMhT, ph, pw, pw - skipW, ph - skipH, ispFwdShift2( lph ), t, LANES, &sumAbs );
        coef = bufA;
      }
      else
      {
        if( ph == 1 ) lds_fwd_pass( bufA, pw, bufB, 1, sMwT, pw, 1, ALL_LINES, pw - skipW, ispFwdShift1( lpw, bd ), t, LANES, &sumAbs );
        else lds_fwd_pass( bufA, ph, bufB, 1, sMhT, ph, 1, ALL_LINES, ph - skipH, ispFwdShift1( lph, bd ), t, LANES, &sumAbs );
        coef = bufB;
      }
      chain_sync<LANES>();
      // Quant::quant and Quant::dequant in place; the levels leave as one TU-shaped block
      for( int i = t; i < partArea; i += LANES )
      {
        const int lv = qr.level( coef[i], absSum );
        if( levels ) levels[( long ) k * partArea + i] = lv;
        coef[i] = qr.dequant( lv );
      }
      chain_sync<LANES>();
      // TrQuant::xIT: columns, then rows; the last pass ends in the clipped reconstruction and its squared error against the original
      auto reconstruct = [&]( int x, int y, int v ) {
        const int at = ( py + y ) * W + px + x, rec = intraClip( ( int ) sReco[at] + v, maxVal ), d = ( int ) sOrg[at] - rec;
        sReco[at] = ( int16_t ) rec;
        sse += ( long long ) ( unsigned long long ) ( ( unsigned ) d * ( unsigned ) d );
      };
      if( pw > 1 && ph > 1 )
      {
        lds_inv_pass( bufA, pw, sMh, ph, pw, pw - skipW, ph - skipH, ispInvShift1(), t, LANES, [bufB]( int o, int, int, int v ) { bufB[o] = v; } );
        chain_sync<LANES>();
        lds_inv_pass( bufB, ph, sMw, pw, ph, ALL_LINES, pw - skipW, ispInvShift2( bd ), t, LANES, [&]( int, int y, int x, int v ) { reconstruct( x, y, v ); } );
      }
      else if( ph == 1 ) lds_inv_pass( bufB, 1, sMw, pw, 1, ALL_LINES, pw - skipW, ispInvShift1D( bd ), t, LANES, [&]( int, int, int x, int v ) { reconstruct( x, 0, v ); } );
      else lds_inv_pass( bufB, 1, sMh, ph, 1, ALL_LINES, ph - skipH, ispInvShift1D( bd ), t, LANES, [&]( int, int, int y, int v ) { reconstruct( 0, y, v ); } );
      long long sums[3] = { sumAbs, absSum, sse };
      chain_reduce_store<LANES, 3>( sums, sRed, sub, t, live, [res, k]( const long long ( &v )[3] ) {
        res->sse[k] = ( uint64_t ) v[2]; res->sumAbs[k] = ( int32_t ) v[0]; res->absSum[k] = ( int32_t ) v[1];
      } );
      chain_sync<LANES>();   // the reconstruction of this TU is what the next region's lines read
    }
  }
  if( live )
  {
    if( t == 0 )
    {
      for( int k = g.numParts; k < ISP_MAX_PARTS; k++ ) { res->sse[k] = 0; res->sumAbs[k] = 0; res->absSum[k] = 0; }
      res->numParts = g.numParts; res->reserved = 0;
    }
    int16_t *reco = recoBase + J.outOff;
    for( int i = t; i < W * H; i += LANES ) reco[i] = sReco[i];
  }
}

IspTabs isp_tabs( const vtmhip_ctx *ctx )
{
  IspTabs t;
  for( int l = 0; l < 7; l++ ) { t.m[0][l] = ctx->trTab[VTMHIP_DCT2][l]; t.m[1][l] = ctx->trTab[VTMHIP_DST7][l]; }
  return t;
}

constexpr size_t ISP_MAX_LDS = 64 * 1024;

// the lanes a job gets: by the largest CU, as the intra prediction kernels; the workgroup also where four (sixteen) jobs would not fit its LDS
int isp_lanes( const IspPlan &plan )
{
  int lanes = intra_lanes( plan.maxArea );
  while( lanes && lanes < 256 && ( size_t ) ( 256 / lanes ) * plan.jobInts * sizeof( int ) > ISP_MAX_LDS ) lanes *= 4;
  return lanes;
}

}   // namespace

extern "C"
{

int vtmhip_isp_struct_size( int which )
{
  switch( which )
  {
  case 0: return ( int ) sizeof( vtmhip_isp_job );
  case 1: return ( int ) sizeof( vtmhip_isp_result );
  case 2: return ( int ) sizeof( vtmhip_isp_geom );
  default: return -1;
  }
}

int vtmhip_isp_geometry( int width, int height, int split, vtmhip_isp_geom *out )
{
  if( !out || !ispCanUse( width, height ) || ( split != ISP_HOR && split != ISP_VER ) ) return VTMHIP_E_INVALID;
  IspGeom g;
  ispGeometry( width, height, split, g );
  out->numParts = g.numParts; out->partW = g.partW; out->partH = g.partH;
  out->numRegions = g.numRegions; out->regW = g.regW; out->regH = g.regH;
  out->typeHor = ispTrType( g.partW ); out->typeVer = ispTrType( g.partH );
  return VTMHIP_OK;
}

// a region some split of the CU has
static bool isp_region_ok( int cuW, int cuH, int regW, int regH )
{
  if( !ispCanUse( cuW, cuH ) ) return false;
  for( int split = ISP_HOR; split <= ISP_VER; split++ )
  {
    IspGeom g;
    ispGeometry( cuW, cuH, split, g );
    if( g.regW == regW && g.regH == regH ) return true;
  }
  return false;
}

int vtmhip_isp_pred_params( int cuW, int cuH, int regW, int regH, int mode, vtmhip_intra_params *out )
{
  if( !out || !isp_region_ok( cuW, cuH, regW, regH ) || mode < 0 || mode >= INTRA_NUM_LUMA_MODE ) return VTMHIP_E_INVALID;
  ispPredParams( cuW, cuH, regW, regH, mode, *out );
  return VTMHIP_OK;
}

int vtmhip_isp_tr_types( int partW, int partH, int *typeHor, int *typeVer )
{
  if( !typeHor || !typeVer || partW < 1 || partW > 64 || partH < 1 || partH > 64 || ( partW & ( partW - 1 ) ) || ( partH & ( partH - 1 ) ) ) return VTMHIP_E_INVALID;
  *typeHor = ispTrType( partW ); *typeVer = ispTrType( partH );
  return VTMHIP_OK;
}

int vtmhip_isp_pred_region_host( int cuW, int cuH, int regW, int regH, int mode, int bitDepth, const int16_t *top, const int16_t *left, int16_t *pred )
{
  if( !top || !left || !pred || !isp_region_ok( cuW, cuH, regW, regH ) || mode < 0 || mode >= INTRA_NUM_LUMA_MODE || bitDepth < 8 || bitDepth > 12 ) return VTMHIP_E_INVALID;
  isp_host::predRegion( cuW, cuH, regW, regH, mode, bitDepth, top, left, pred, regW );
  return VTMHIP_OK;
}

int vtmhip_isp_next_lines_host( int cuW, int cuH, int split, int region, int sideAvail, const int16_t *top, const int16_t *left, const int16_t *reco, int16_t *topOut,
                                int16_t *leftOut )
{
  if( !top || !left || !reco || !topOut || !leftOut || !ispCanUse( cuW, cuH ) || ( split != ISP_HOR && split != ISP_VER ) || sideAvail < 0 || sideAvail > 1 )
    return VTMHIP_E_INVALID;
  IspGeom g;
  ispGeometry( cuW, cuH, split, g );
  if( region < 1 || region >= g.numRegions ) return VTMHIP_E_INVALID;
  const IspLines l = { top, left, reco, cuW, split, sideAvail };
  isp_host::nextLines( l, g, cuW, cuH, region, topOut, leftOut );
  return VTMHIP_OK;
}

int vtmhip_isp_chain_host( const int16_t *refBase, const int16_t *orgBase, const vtmhip_intra_block *blocks, int numBlocks, const vtmhip_isp_job *jobs, int n,
                           int16_t *predBase, int32_t *levelsBase, int16_t *recoBase, vtmhip_isp_result *results )
{
  if( n < 0 || numBlocks < 0 ) return VTMHIP_E_INVALID;
  if( n == 0 ) return VTMHIP_OK;
  if( !refBase || !orgBase || !blocks || !jobs || !recoBase || !results ) return VTMHIP_E_INVALID;
  IspPlan plan;
  if( !ispScan( blocks, numBlocks, jobs, n, plan ) ) return VTMHIP_E_INVALID;
  for( int i = 0; i < n; i++ ) isp_host::chainJob( refBase, orgBase, blocks[jobs[i].block], jobs[i], predBase, levelsBase, recoBase, results[i] );
  return VTMHIP_OK;
}

int vtmhip_isp_chain_lanes_host( const vtmhip_intra_block *blocks, int numBlocks, const vtmhip_isp_job *jobs, int n, int *lanes )
{
  if( n <= 0 || numBlocks < 0 || !blocks || !jobs || !lanes ) return VTMHIP_E_INVALID;
  IspPlan plan;
  if( !ispScan( blocks, numBlocks, jobs, n, plan ) ) return VTMHIP_E_INVALID;
  *lanes = isp_lanes( plan );
  return VTMHIP_OK;
}

int vtmhip_isp_chain_batch_dev( vtmhip_ctx *ctx, const int16_t *d_refBase, const int16_t *d_orgBase, const vtmhip_intra_block *d_blocks, int numBlocks,
                                const vtmhip_isp_job *d_jobs, int n, int16_t *d_predBase, int32_t *d_levelsBase, int16_t *d_recoBase, vtmhip_isp_result *d_results )
{
  VTMHIP_CHECK_CTX( ctx );
  VTMHIP_REQUIRE( ctx, numBlocks >= 0, "numBlocks" );
  VTMHIP_BATCH_ARGS( ctx, n, d_refBase && d_orgBase && d_blocks && d_jobs && d_recoBase && d_results );
  // the kernel trusts its tables: both are read back and checked before anything runs
  HostStage    hs( ctx );
  const size_t bBlk = ( size_t ) numBlocks * sizeof( vtmhip_intra_block ), bJob = ( size_t ) n * sizeof( vtmhip_isp_job );
  const size_t oBlk = hs.region( bBlk ), oJob = hs.region( bJob );
  VTMHIP_TRY( hs.reserve() );
  VTMHIP_TRY( hs.pull( oBlk, d_blocks, bBlk ) );
  VTMHIP_TRY( hs.pull( oJob, d_jobs, bJob ) );
  VTMHIP_TRY( hs.sync() );
  IspPlan plan;
  VTMHIP_REQUIRE( ctx, ispScan( hs.host<vtmhip_intra_block>( oBlk ), numBlocks, hs.host<vtmhip_isp_job>( oJob ), n, plan ),
                  "ISP chain tables: sides 4..64 without 4x4, bitDepth 8..12, multiRefIdx 0, block index, mode 0..66, split 1..2, sideAvail / isIRAP 0..1, qpRem 0..5, "
                  "qpPer >= 0, reserved fields 0" );
  VTMHIP_TRY( vtmhip_internal_tr_tables( ctx ) );
  const IspTabs tabs = isp_tabs( ctx );
  const int     lanes = isp_lanes( plan ), perGroup = 256 / lanes;
  const size_t  lds = ( size_t ) perGroup * plan.jobInts * sizeof( int );
  VTMHIP_REQUIRE( ctx, lds <= ISP_MAX_LDS, "ISP chain: LDS plan" );
  const dim3 grid( ( n + perGroup - 1 ) / perGroup );
  VTMHIP_TIME_KERNEL( ctx, "isp_chain_kernel" );
  if( lanes == 16 )
    hipLaunchKernelGGL( isp_chain_kernel<16>, grid, dim3( 256 ), lds, ctx->stream, d_refBase, d_orgBase, d_blocks, d_jobs, n, tabs, plan, d_predBase, d_levelsBase, d_recoBase,
                        d_results );
  else if( lanes == 64 )
    hipLaunchKernelGGL( isp_chain_kernel<64>, grid, dim3( 256 ), lds, ctx->stream, d_refBase, d_orgBase, d_blocks, d_jobs, n, tabs, plan, d_predBase, d_levelsBase, d_recoBase,
                        d_results );
  else
    hipLaunchKernelGGL( isp_chain_kernel<256>, grid, dim3( 256 ), lds, ctx->stream, d_refBase, d_orgBase, d_blocks, d_jobs, n, tabs, plan, d_predBase, d_levelsBase, d_recoBase,
                        d_results );
  VTMHIP_LAUNCHED( ctx );
  return VTMHIP_OK;
}

}   // extern "C"
