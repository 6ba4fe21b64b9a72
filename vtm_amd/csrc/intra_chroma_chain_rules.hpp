// intra_chroma_chain_rules.hpp -- the tables of vtmhip_intra_chroma_chain_batch_dev, defined once for host and device: plain integer functions without a HIP
// dependency, so host/test_intra_chroma_chain.cpp compiles them with g++ and the expansion kernel of intra_chroma_chain.hip uses the same text.
//   ichainBlockOk       what a vtmhip_intra_chroma_block must satisfy: cclmBlockOk, the rule the prediction kernel skips by, and reserved bytes of 0
//   ichainTuOk          what a vtmhip_intra_chroma_tu_job must satisfy
//   ichainJointOk       what a vtmhip_intra_chroma_joint_job must satisfy
//   ichainExpandTu      the single job as a vtmhip_tu_job of the fused chain: the residual of its component at stride W, shape and bit depth from the block
//   ichainExpandJoint   the joint job as a vtmhip_jccr_job of the joint chain: both residuals of its prediction
//   ichainScan          the host pass over all four tables: every entry is checked, and the launch plan falls out of the same walk (chain_rules.hpp's ChainShapes
//                       per job table)
// A table with one malformed entry is rejected whole: the chain kernels trust their jobs.
#pragma once
#include "chain_rules.hpp"
#include "cclm_rules.hpp"

#if defined( __HIPCC__ )
#define ICCHAIN_HD __host__ __device__ inline
#else
#define ICCHAIN_HD inline
#endif

struct IchainPlan
{
  int maxBlockArea;              // over the block table: decides the lanes a prediction job gets
  ChainShapes tu, joint;         // over the single jobs, over the joint jobs (chain_rules.hpp)
  int anyLm;                     // some prediction job is an LM mode: the luma plane is read
  int crs;                       // some job has a non-zero adj: the CRS instantiations of the chains are dispatched
};

ICCHAIN_HD bool ichainBlockOk( const vtmhip_intra_chroma_block &b )
{
  const CclmAvail v = { b.above, b.left, b.aboveRight, b.belowLeft, b.firstRow, b.colocated };
  return cclmBlockOk( b.width, b.height, b.bitDepth, v ) && !b.reserved[0] && !b.reserved[1] && !b.reserved[2];
}

ICCHAIN_HD bool ichainTrOk( int typeHor ) { return typeHor == VTMHIP_DCT2 || typeHor == VTMHIP_TRSKIP; }   // chroma sides end at 32: transform skip fits every block

ICCHAIN_HD bool ichainTuOk( const vtmhip_intra_chroma_tu_job &t )
{
  return t.component <= 1 && ichainTrOk( t.typeHor ) && chainQpOk( t.qpPer, t.qpRem ) && t.chromaAdj <= 32767 && t.reserved == 0 && t.pad == 0;
}

ICCHAIN_HD bool ichainJointOk( const vtmhip_intra_chroma_joint_job &t )
{
  return t.cbfMask >= 1 && t.cbfMask <= 3 && t.signFlag <= 1 && ichainTrOk( t.typeHor ) && chainQpOk( t.qpPer, t.qpRem ) && t.chromaAdj <= 32767 && t.pad == 0;
}

ICCHAIN_HD void ichainExpandTu( const vtmhip_intra_chroma_tu_job &t, const vtmhip_intra_chroma_block &b, const vtmhip_intra_chroma_job &p, vtmhip_tu_job &out )
{
  out.resiOff    = t.component ? p.crPredOff : p.cbPredOff;
  out.outOff     = t.outOff;
  out.resiStride = b.width;
  out.width = b.width; out.height = b.height;
  out.qpPer = t.qpPer; out.qpRem = t.qpRem;
  out.typeHor = t.typeHor; out.typeVer = t.typeHor;
  out.bitDepth = b.bitDepth; out.isIRAP = t.isIRAP;
  out.pad = 0; out.chromaAdj = t.chromaAdj;
}

ICCHAIN_HD void ichainExpandJoint( const vtmhip_intra_chroma_joint_job &t, const vtmhip_intra_chroma_block &b, const vtmhip_intra_chroma_job &p, vtmhip_jccr_job &out )
{
  out.cbOff = p.cbPredOff; out.crOff = p.crPredOff;
  out.outOff     = t.outOff;
  out.resiStride = b.width;
  out.width = b.width; out.height = b.height;
  out.qpPer = t.qpPer; out.qpRem = t.qpRem;
  out.typeHor = t.typeHor; out.bitDepth = b.bitDepth; out.isIRAP = t.isIRAP;
  out.cbfMask = t.cbfMask; out.signFlag = t.signFlag;
  out.reserved0 = 0; out.chromaAdj = t.chromaAdj;
  out.reserved1[0] = out.reserved1[1] = out.reserved1[2] = out.reserved1[3] = 0;
}

// false: an entry the prediction entry would skip or the chains must not see
inline bool ichainScan( const vtmhip_intra_chroma_block *blocks, int numBlocks, const vtmhip_intra_chroma_job *jobs, int nPred, const vtmhip_intra_chroma_tu_job *tuJobs,
                        int nTu, const vtmhip_intra_chroma_joint_job *jointJobs, int nJoint, IchainPlan &plan )
{
  plan = IchainPlan();
  for( int i = 0; i < numBlocks; i++ )
  {
    if( !ichainBlockOk( blocks[i] ) ) return false;
    if( blocks[i].width * blocks[i].height > plan.maxBlockArea ) plan.maxBlockArea = blocks[i].width * blocks[i].height;
  }
  for( int i = 0; i < nPred; i++ )
  {
    const vtmhip_intra_chroma_job &j = jobs[i];
    if( j.block < 0 || j.block >= numBlocks || !cclmModeOk( j.mode ) || j.reserved[0] || j.reserved[1] || j.reserved[2] ) return false;
    if( cclmIsLm( j.mode ) ) plan.anyLm = 1;
  }
  plan.tu.begin( nTu );
  for( int i = 0; i < nTu; i++ )
  {
    const vtmhip_intra_chroma_tu_job &t = tuJobs[i];
    if( t.pred < 0 || t.pred >= nPred || !ichainTuOk( t ) ) return false;
    const vtmhip_intra_chroma_block &b = blocks[jobs[t.pred].block];
    plan.tu.add( i, b.width, b.height, t.typeHor );
    if( t.chromaAdj ) plan.crs = 1;
  }
  plan.joint.begin( nJoint );
  for( int i = 0; i < nJoint; i++ )
  {
    const vtmhip_intra_chroma_joint_job &t = jointJobs[i];
    if( t.pred < 0 || t.pred >= nPred || !ichainJointOk( t ) ) return false;
    const vtmhip_intra_chroma_block &b = blocks[jobs[t.pred].block];
    plan.joint.add( i, b.width, b.height, t.typeHor );
    if( t.chromaAdj ) plan.crs = 1;
  }
  return true;
}

// vtmhip_intra_chroma_chain_make_jobs without its NULL checks: outTu[i] / outJoint[i] = job i as its chain sees it; nothing is written when a table is rejected
inline bool ichainMakeJobs( const vtmhip_intra_chroma_block *blocks, int numBlocks, const vtmhip_intra_chroma_job *jobs, int nPred, const vtmhip_intra_chroma_tu_job *tuJobs,
                            int nTu, const vtmhip_intra_chroma_joint_job *jointJobs, int nJoint, vtmhip_tu_job *outTu, vtmhip_jccr_job *outJoint, IchainPlan &plan )
{
  if( !ichainScan( blocks, numBlocks, jobs, nPred, tuJobs, nTu, jointJobs, nJoint, plan ) ) return false;
  for( int i = 0; i < nTu; i++ ) ichainExpandTu( tuJobs[i], blocks[jobs[tuJobs[i].pred].block], jobs[tuJobs[i].pred], outTu[i] );
  for( int i = 0; i < nJoint; i++ ) ichainExpandJoint( jointJobs[i], blocks[jobs[jointJobs[i].pred].block], jobs[jointJobs[i].pred], outJoint[i] );
  return true;
}
