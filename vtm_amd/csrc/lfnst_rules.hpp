// lfnst_rules.hpp -- the rules of the LFNST residual chain (vtmhip_lfnst_chain_batch_dev, vtmhip_intra_chain_lfnst_batch_dev), defined once for host and device: plain
// integer functions without a HIP dependency, so host/test_lfnst_chain.cpp compiles them with g++ and the kernels of lfnst_chain.hip use the same text.
//   lfnstWideAngle      PU::getWideAngle                                             CommonLib/UnitTools.cpp:733-759
//   lfnstIntraMode      TrQuant::getLFNSTIntraMode, lfnstTranspose: getTransposeFlag  CommonLib/TrQuant.cpp:313-337
//   lfnstSetOfWide      g_lfnstLut[ getLFNSTIntraMode( . ) ] = lfnstTrSetIdx of H.266 8.7.4.1, written as ranges of the wide-angle mode
//   lfnstModeOf         set index and transpose flag of a prediction (MIP: planar, TrQuant.cpp:452-455)
//   lfnstKeep / lfnstZeroOut / lfnstTrSize   the kept primary region (TrQuant.cpp:792-804, :872-884), the quantised scan positions (Quant.cpp:1003-1009)
//   lfnstScanPos        scan position k -> x + y * width: the rule of vtmhip_lfnst_scan_host
//   lfnstRegionXY       entry v of the core multiply's vector -> (x, y) of the region (TrQuant.cpp:474-511)
//   lfnstChainJobOk     what a vtmhip_lfnst_chain_job must satisfy;  lfnstChainScan: the host pass over such a table
//   lfnstTuOk / lfnstExpand / lfnstLevelScan / lfnstLevelMakeJobs   the LFNST table of the intra level entry, beside intra_chain_rules.hpp's (whose expansion loop
//                       fills the plain jobs here too); the quantiser check is chain_rules.hpp's
// PU::getWideAngle is NOT IntraPrediction::getModifiedWideAngle (intraWideAngle): a tall block's modes next to 66 go down by 67 there, by 65 here, so that 0 and 1
// stay planar and DC.  lfnstWideAngle takes intraWideAngle and corrects the tall case.
#pragma once
#include "intra_chain_rules.hpp"

#if defined( __HIPCC__ )
#define LFNST_HD __host__ __device__ inline
#else
#define LFNST_HD inline
#endif

LFNST_HD int lfnstWideAngle( int w, int h, int mode )
{
  const int wide = intraWideAngle( w, h, mode );
  return ( h > w && wide != mode ) ? wide - 2 : wide;
}

LFNST_HD int  lfnstIntraMode( int wide ) { return wide < 0 ? wide + 14 + INTRA_NUM_LUMA_MODE : wide >= INTRA_NUM_LUMA_MODE ? wide + 14 : wide; }   // NUM_EXT_LUMA_MODE >> 1 = 14
LFNST_HD bool lfnstTranspose( int intraMode ) { return intraMode >= INTRA_NUM_LUMA_MODE ? intraMode >= INTRA_NUM_LUMA_MODE + 14 : intraMode > INTRA_DIA; }

LFNST_HD int lfnstSetOfWide( int wide )
{
  if( wide < 0 ) return 1;
  if( wide <= 1 ) return 0;
  if( wide <= 12 ) return 1;
  if( wide <= 23 ) return 2;
  if( wide <= 44 ) return 3;
  if( wide <= 55 ) return 2;
  return 1;   // 56 .. 80
}

LFNST_HD void lfnstModeOf( int w, int h, int mode, bool isMip, int &setIdx, int &transpose )
{
  const int wide = isMip ? INTRA_PLANAR : lfnstWideAngle( w, h, mode );
  setIdx    = lfnstSetOfWide( wide );
  transpose = lfnstTranspose( lfnstIntraMode( wide ) );
}

LFNST_HD bool lfnstSideOk( int s ) { return intraSideOk( s ); }   // 4 .. 64
LFNST_HD bool lfnstShapeOk( int w, int h, bool isMip ) { return lfnstSideOk( w ) && lfnstSideOk( h ) && ( !isMip || ( w >= 16 && h >= 16 ) ); }   // allowLfnstWithMip, UnitTools.cpp:3902

LFNST_HD int lfnstKeep( int w, int h ) { return ( w >= 8 && h >= 8 ) ? 8 : 4; }                                     // the side of the kept primary region
LFNST_HD int lfnstZeroOut( int w, int h ) { return ( ( w == 4 && h == 4 ) || ( w == 8 && h == 8 ) ) ? 8 : 16; }     // = the number of quantised scan positions
LFNST_HD int lfnstTrSize( int w, int h ) { return ( w >= 8 && h >= 8 ) ? 48 : 16; }

// inside a 4x4 group: up-right diagonals, each from bottom-left to top-right; the groups of the 8x8 region in the same order: (0,0), (0,1), (1,0), (1,1)
LFNST_HD int lfnstScanPos( int k, int width, bool sb8 )
{
  // dx = 0 0 1 0 1 2 0 1 2 3 1 2 3 2 3 3 and dy = 0 1 0 2 1 0 3 2 1 0 3 2 1 3 2 3, two bits per entry from the low end (a word, not an array a kernel would index)
  const int g = k >> 4, i = k & 15, dx = ( int ) ( ( 0xfb9e4910u >> ( 2 * i ) ) & 3 ), dy = ( int ) ( ( 0xedb1b184u >> ( 2 * i ) ) & 3 );
  const int gx = sb8 ? ( g == 2 || g == 3 ) : 0, gy = sb8 ? ( g == 1 || g == 3 ) : 0;
  return ( gx * 4 + dx ) + ( gy * 4 + dy ) * width;
}

// rows 0 .. 3 of the region are 4 or 8 wide, rows 4 .. 7 of the 8x8 region 4 wide; transposed: the vector index of (x, y) is that of (y, x)
LFNST_HD void lfnstRegionXY( int v, bool sb8, bool transpose, int &x, int &y )
{
  int row, col;
  if( !sb8 ) { row = v >> 2; col = v & 3; }
  else if( v < 32 ) { row = v >> 3; col = v & 7; }
  else { row = 4 + ( ( v - 32 ) >> 2 ); col = ( v - 32 ) & 3; }
  if( transpose ) { x = row; y = col; } else { x = col; y = row; }
}

// ---- the chain's own table ---------------------------------------------------------------------------------------------------------------------------------
LFNST_HD bool lfnstChainJobOk( const vtmhip_lfnst_chain_job &j )
{
  for( int i = 0; i < 7; i++ )
    if( j.pad[i] ) return false;
  return lfnstSideOk( j.width ) && lfnstSideOk( j.height ) && j.resiStride >= j.width && j.bitDepth >= 8 && j.bitDepth <= 12 && chainQpOk( j.qpPer, j.qpRem ) &&
         j.setIdx <= 3 && j.index <= 1 && j.transpose <= 1;
}

// what one job needs of LDS, in ints: the int16 residual in rows of W + 2 (an odd number of words: a column read meets no bank twice), the first pass's
// keep x ( H + 1 ) block, keep rows of both core matrices (int16), the region (64), the core multiply's vector (48), the dequantised 16 and the levels of the
// top-left 4x4 (16)
LFNST_HD int lfnstJobInts( int w, int h )
{
  const int keep = lfnstKeep( w, h );
  return ( ( ( w + 2 ) * h ) >> 1 ) + keep * ( h + 1 ) + ( ( keep * ( w + h ) ) >> 1 ) + 64 + 48 + 16 + 16;
}

LFNST_HD int lfnstLanes( int maxArea ) { return maxArea <= 256 ? 16 : 64; }   // lanes per job: sixteen jobs per workgroup up to 256 samples, a wave per job above

struct LfnstPlan
{
  int maxArea;   // over the jobs (0 without any): decides the lanes per job
  int jobInts;   // the largest lfnstJobInts
};

LFNST_HD void lfnstPlanAdd( LfnstPlan &plan, int w, int h )
{
  if( w * h > plan.maxArea ) plan.maxArea = w * h;
  if( lfnstJobInts( w, h ) > plan.jobInts ) plan.jobInts = lfnstJobInts( w, h );
}

inline bool lfnstChainScan( const vtmhip_lfnst_chain_job *jobs, int n, LfnstPlan &plan )
{
  plan.maxArea = plan.jobInts = 0;
  for( int i = 0; i < n; i++ )
  {
    if( !lfnstChainJobOk( jobs[i] ) ) return false;
    lfnstPlanAdd( plan, jobs[i].width, jobs[i].height );
  }
  return true;
}

// ---- the LFNST table of the intra level entry ------------------------------------------------------------------------------------------------------------------
LFNST_HD bool lfnstTuOk( const vtmhip_intra_lfnst_tu_job &t, int w, int h, bool isMip )
{
  return t.lfnstIdx >= 1 && t.lfnstIdx <= 2 && chainQpOk( t.qpPer, t.qpRem ) && t.reserved[0] == 0 && t.reserved[1] == 0 && t.pad == 0 && lfnstShapeOk( w, h, isMip );
}

// mode: the regular mode of the prediction (ignored for MIP)
LFNST_HD void lfnstExpand( const vtmhip_intra_lfnst_tu_job &t, const vtmhip_intra_block &b, int64_t predOff, bool isMip, int mode, vtmhip_lfnst_chain_job &out )
{
  int setIdx, transpose;
  lfnstModeOf( b.width, b.height, mode, isMip, setIdx, transpose );
  out.resiOff    = predOff;
  out.outOff     = t.outOff;
  out.resiStride = b.width;
  out.width = b.width; out.height = b.height;
  out.qpPer = t.qpPer; out.qpRem = t.qpRem;
  out.bitDepth = b.bitDepth; out.isIRAP = t.isIRAP;
  out.setIdx = ( uint8_t ) setIdx; out.index = ( uint8_t ) ( t.lfnstIdx - 1 ); out.transpose = ( uint8_t ) transpose;
  for( int i = 0; i < 7; i++ ) out.pad[i] = 0;
}

// job i of the LFNST table as the chain sees it; the tables have passed intraChainScan and lfnstLevelScan
LFNST_HD void lfnstExpandAt( const vtmhip_intra_block *blocks, const vtmhip_intra_job *intraJobs, int nIntra, const vtmhip_mip_job *mipJobs, const vtmhip_intra_lfnst_tu_job &t,
                             vtmhip_lfnst_chain_job &out, int &block )
{
  int64_t predOff;
  intraChainPred( intraJobs, nIntra, mipJobs, t.pred, block, predOff );
  const bool isMip = t.pred >= nIntra;
  lfnstExpand( t, blocks[block], predOff, isMip, isMip ? 0 : intraJobs[t.pred].mode, out );
}

// the host pass over the LFNST table; the other four tables have passed intraChainScan
inline bool lfnstLevelScan( const vtmhip_intra_block *blocks, const vtmhip_intra_job *intraJobs, int nIntra, const vtmhip_mip_job *mipJobs, int nMip,
                            const vtmhip_intra_lfnst_tu_job *lfnstJobs, int nLfnst, LfnstPlan &plan )
{
  plan.maxArea = plan.jobInts = 0;
  for( int i = 0; i < nLfnst; i++ )
  {
    const vtmhip_intra_lfnst_tu_job &t = lfnstJobs[i];
    if( t.pred < 0 || t.pred >= nIntra + nMip ) return false;
    int     blk;
    int64_t predOff;
    intraChainPred( intraJobs, nIntra, mipJobs, t.pred, blk, predOff );
    const int w = blocks[blk].width, h = blocks[blk].height;
    if( !lfnstTuOk( t, w, h, t.pred >= nIntra ) ) return false;
    lfnstPlanAdd( plan, w, h );
  }
  return true;
}

// vtmhip_intra_chain_lfnst_make_jobs without its NULL checks: nothing is written when a table is rejected
inline bool lfnstLevelMakeJobs( const vtmhip_intra_block *blocks, int numBlocks, const vtmhip_intra_job *intraJobs, int nIntra, const vtmhip_mip_job *mipJobs, int nMip,
                                const vtmhip_intra_tu_job *tuJobs, int nTu, const vtmhip_intra_lfnst_tu_job *lfnstJobs, int nLfnst, vtmhip_tu_job *outTu,
                                vtmhip_lfnst_chain_job *outLfnst, IntraChainPlan &plan, LfnstPlan &lplan )
{
  if( !intraChainScan( blocks, numBlocks, intraJobs, nIntra, mipJobs, nMip, tuJobs, nTu, plan ) ) return false;
  if( !lfnstLevelScan( blocks, intraJobs, nIntra, mipJobs, nMip, lfnstJobs, nLfnst, lplan ) ) return false;
  intraChainExpandAll( blocks, intraJobs, nIntra, mipJobs, tuJobs, nTu, outTu );
  for( int i = 0; i < nLfnst; i++ )
  {
    int blk;
    lfnstExpandAt( blocks, intraJobs, nIntra, mipJobs, lfnstJobs[i], outLfnst[i], blk );
  }
  return true;
}
