// isp_rules.hpp -- the rules of intra sub-partitions (ISP) of the reference, defined once for host and device on top of intra_rules.hpp: plain integer functions
// without a HIP dependency, so host/test_isp.cpp compiles them with g++ and the kernel of isp_chain.hip uses the same text.
//   ispCanUse            CU::canUseISP with MaxTbSize 64                                                   CommonLib/UnitTools.cpp:400-409
//   ispSplitDim          CU::getISPSplitDim                                                                :433-455
//   ispGeometry          the sub-partitions (TUs) of a CU and its prediction regions: CU::isPredRegDiffFromTB, isMinWidthPredEnabledForBlkSize,
//                        isFirstTBInPredReg, adjustPredArea                                                :3609-3630
//   ispPredParams        IntraPrediction::initPredIntraParams with cu->ispMode set                         CommonLib/IntraPrediction.cpp:356-444
//   ispSideAt / ispMainAt   the two lines a prediction region behind the first sees: IntraPrediction::initIntraPatternChTypeISP, both splits, both
//                        availability branches                                                             :837-910
//   ispTrType            TrQuant::getTrTypes for an ISP TU                                                 CommonLib/TrQuant.cpp:713-724
//   ispFwdShift1 ...     the shifts of TrQuant::xT / xIT, two passes or the one pass of a TU with a side of 1   :826-850, :888-911
//   ispBlockOk / ispJobOk / ispScan   what the tables of vtmhip_isp_chain_batch_dev must satisfy, shared with vtmhip_isp_chain_host
//
// A CU of W x H is split (1: horizontally, into rows; 2: vertically, into columns -- ISPType) into numParts TUs of partW x partH.  A prediction region is a TU,
// except under a vertical split of a CU of width 4, or of width 8 and height above 4: there the TUs are 1 or 2 wide and the region is 4 wide, predicted once before
// any of its TUs is reconstructed.  Regions and TUs follow each other along the split; `ext` is a region's extent in that direction.
//
// The lines.  Region 0 predicts from the CU's own lines, top[0 .. 2W] and left[0 .. 2H] (:819-831).  Region r > 0 sees (horizontal split; the vertical one is its
// transpose): the side line shifted by r * ext -- the reference shifts by ext in place per region (:851-854), which inside the range a region reads, 0 .. H + ext, is the
// CU's line at idx + r * ext -- or, when the neighbour on that side does not exist, the first sample of the reconstruction row above the region everywhere (:858-861);
// the main line from that row, its last sample repeated to W + regW (:863-874); the corner from the (new) side line.  These are reads over (CU lines,
// reconstruction), ispSideAt / ispMainAt; a prediction reads a line up to its end, W + regW and H + regH (m_topRefLength / m_leftRefLength :834-841), through IspBlk.
#pragma once
#include "chain_rules.hpp"
#include "intra_rules.hpp"

#if defined( __HIPCC__ )
#define ISP_HD __host__ __device__ inline
#else
#define ISP_HD inline
#endif

enum { ISP_HOR = 1, ISP_VER = 2, ISP_MAX_PARTS = 4, ISP_PRED_REG_MIN_WIDTH = 4 };

struct IspGeom
{
  int numParts, partW, partH;     // the TUs
  int numRegions, regW, regH;     // the prediction regions
  int ext, tusPerRegion;          // a region's extent along the split; numParts / numRegions
};

ISP_HD bool ispCanUse( int w, int h ) { return intraSideOk( w ) && intraSideOk( h ) && intraLog2( w ) + intraLog2( h ) > 4; }   // MIN_TB_SIZEY 4; sides up to MaxTbSize 64

ISP_HD int ispSplitDim( int w, int h, int split )
{
  const int splitDim = split == ISP_HOR ? h : w, other = split == ISP_HOR ? w : h;
  const int factor = other < 16 ? 16 >> intraLog2( other ) : 1;   // a TU has at least 16 samples
  return ( splitDim >> 2 ) < factor ? factor : splitDim >> 2;
}

ISP_HD void ispGeometry( int w, int h, int split, IspGeom &g )
{
  const int dim = ispSplitDim( w, h, split );
  if( split == ISP_HOR ) { g.partW = w; g.partH = dim; g.numParts = h / dim; }
  else { g.partW = dim; g.partH = h; g.numParts = w / dim; }
  g.regW = g.partW; g.regH = g.partH;
  if( split == ISP_VER && ( w == 4 || ( w == 8 && h > 4 ) ) && g.regW < ISP_PRED_REG_MIN_WIDTH ) g.regW = ISP_PRED_REG_MIN_WIDTH;
  g.ext          = split == ISP_HOR ? g.regH : g.regW;
  g.numRegions   = ( split == ISP_HOR ? h : w ) / g.ext;
  g.tusPerRegion = g.numParts / g.numRegions;
}

// the rectangle of TU k inside the CU
ISP_HD void ispPartRect( const IspGeom &g, int split, int k, int &x, int &y )
{
  x = split == ISP_HOR ? 0 : k * g.partW;
  y = split == ISP_HOR ? k * g.partH : 0;
}

ISP_HD void ispPredParams( int cuW, int cuH, int regW, int regH, int mode, vtmhip_intra_params &p ) { intraPredParams( regW, regH, mode, 0, p, false, cuW, cuH ); }

// DST7 on a side of 4 .. 16, else DCT2 (a side of 1 is not transformed at all)
ISP_HD int ispTrType( int side ) { return side >= 4 && side <= 16 ? VTMHIP_DST7 : VTMHIP_DCT2; }
ISP_HD int ispTrSkip( int side ) { return side > 32 ? side - 32 : 0; }   // the zero-out of the 64-point DCT2; DST7 stops at 16 here

// a TU with both sides above 1: first (horizontal) and second forward shift, first (vertical) and second inverse shift; a TU with a side of 1: its one pass
ISP_HD int ispFwdShift1( int log2N, int bitDepth ) { return log2N + bitDepth + 6 - 15; }
ISP_HD int ispFwdShift2( int log2N ) { return log2N + 6; }
ISP_HD int ispInvShift1() { return 7; }
ISP_HD int ispInvShift2( int bitDepth ) { return 6 + 15 - 1 - bitDepth; }
ISP_HD int ispInvShift1D( int bitDepth ) { return ispInvShift2( bitDepth ) + 1; }

// the block as a prediction region sees it: the lines end where the reference's lengths say, not at twice the region's sides
struct IspBlk : IntraBlk
{
  int topLast, leftLast;
};
ISP_HD int intraTopLast( const IspBlk &b ) { return b.topLast; }
ISP_HD int intraLeftLast( const IspBlk &b ) { return b.leftLast; }

// what the line reads of a region behind the first go through
struct IspLines
{
  const int16_t *top, *left;   // the CU's lines, 2W + 1 and 2H + 1 samples
  const int16_t *reco;         // the reconstruction so far, W x H at recoStride
  int recoStride, split, sideAvail;
};

// every read of the line update: ISP_READ_CHECK lets host/test_isp.cpp see each index before it is used (the CU's side line ends at twice the CU's side, the
// reconstruction at W * H - 1 when its stride is W)
#ifndef ISP_READ_CHECK
#define ISP_READ_CHECK( idx, last )
#endif
ISP_HD int ispAt( const int16_t *a, int idx, int last )
{
  ISP_READ_CHECK( idx, last );
  return a[idx];
}

// sample idx of the side line (left under a horizontal split, top under a vertical one) of region r > 0
ISP_HD int ispSideAt( const IspLines &l, const IspGeom &g, int r, int idx )
{
  const int off = r * g.ext, cuSide = g.numRegions * g.ext, recoLast = ( l.split == ISP_HOR ? ( cuSide - 1 ) * l.recoStride + g.regW : ( g.regH - 1 ) * l.recoStride + cuSide ) - 1;
  if( l.sideAvail ) return ispAt( l.split == ISP_HOR ? l.left : l.top, idx + off, 2 * cuSide );
  return ispAt( l.reco, l.split == ISP_HOR ? ( off - 1 ) * l.recoStride : off - 1, recoLast );
}

// sample idx of the main line (top under a horizontal split, left under a vertical one) of region r > 0: the corner, the reconstruction next to the region, its last
// sample from there on
ISP_HD int ispMainAt( const IspLines &l, const IspGeom &g, int r, int idx )
{
  if( idx == 0 ) return ispSideAt( l, g, r, 0 );
  const int off = r * g.ext, len = l.split == ISP_HOR ? g.regW : g.regH, i = idx - 1 < len ? idx - 1 : len - 1, cuSide = g.numRegions * g.ext;
  const int recoLast = ( l.split == ISP_HOR ? ( cuSide - 1 ) * l.recoStride + g.regW : ( g.regH - 1 ) * l.recoStride + cuSide ) - 1;
  return ispAt( l.reco, l.split == ISP_HOR ? ( off - 1 ) * l.recoStride + i : i * l.recoStride + off - 1, recoLast );
}

// ---- the tables of vtmhip_isp_chain_batch_dev ---------------------------------------------------------------------------------------------------------------
ISP_HD bool ispBlockOk( const vtmhip_intra_block &b )
{
  return ispCanUse( b.width, b.height ) && b.bitDepth >= 8 && b.bitDepth <= 12 && b.multiRefIdx == 0 && b.reserved[0] == 0 && b.reserved[1] == 0;
}

ISP_HD bool ispJobOk( const vtmhip_isp_job &j, int numBlocks )
{
  return j.block >= 0 && j.block < numBlocks && j.mode < INTRA_NUM_LUMA_MODE && ( j.split == ISP_HOR || j.split == ISP_VER ) && j.sideAvail <= 1 && j.isIRAP <= 1 &&
         chainQpOk( j.qpPer, j.qpRem ) && j.reserved[0] == 0 && j.reserved[1] == 0 && j.reserved[2] == 0 && j.reserved[3] == 0;
}

// what the launch needs to know of a table: the lanes a job gets and the room a job takes in LDS
struct IspPlan
{
  int maxArea;       // over the blocks the jobs name
  int line;          // int16 per line array: twice the longest side + 1, rounded up to even
  int partArea;      // the largest TU
  int mat;           // the largest partW^2 + partH^2: one orientation of the two core matrices (a side of 1 has none)
  int jobInts;       // ints of LDS per job
};

ISP_HD int ispMatInts16( int pw, int ph ) { return ( pw > 1 ? pw * pw : 0 ) + ( ph > 1 ? ph * ph : 0 ); }

// per job: two int blocks of a TU, the original and the reconstruction (int16), four lines (the CU's two, the two a later region sees), the matrices in both orientations
ISP_HD int ispJobInts( const IspPlan &p ) { return 2 * p.partArea + ( 2 * p.maxArea + 4 * p.line + 2 * p.mat ) / 2; }

// false: a malformed table -- a shape canUseISP refuses, a bit depth outside 8 .. 12, multiRefIdx != 0 or a non-zero reserved field in a block a job names or anywhere
// in the block table; a mode above 66, a split outside 1 .. 2, flags above 1, QP fields out of range, non-zero reserved fields or a block index outside the table in a job
inline bool ispScan( const vtmhip_intra_block *blocks, int numBlocks, const vtmhip_isp_job *jobs, int n, IspPlan &plan )
{
  plan.maxArea = plan.line = plan.partArea = plan.mat = 0;
  for( int i = 0; i < numBlocks; i++ )
    if( !ispBlockOk( blocks[i] ) ) return false;
  for( int i = 0; i < n; i++ )
  {
    if( !ispJobOk( jobs[i], numBlocks ) ) return false;
    const vtmhip_intra_block &b = blocks[jobs[i].block];
    IspGeom g;
    ispGeometry( b.width, b.height, jobs[i].split, g );
    const int side = b.width > b.height ? b.width : b.height, line = 2 * side + 2, mat = ispMatInts16( g.partW, g.partH );
    if( b.width * b.height > plan.maxArea ) plan.maxArea = b.width * b.height;
    if( line > plan.line ) plan.line = line;
    if( g.partW * g.partH > plan.partArea ) plan.partArea = g.partW * g.partH;
    if( mat > plan.mat ) plan.mat = mat;
  }
  plan.jobInts = ispJobInts( plan );
  return true;
}
