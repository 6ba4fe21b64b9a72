// intra_chain_rules.hpp -- the tables of vtmhip_intra_chain_batch_dev, defined once for host and device: plain integer functions without a HIP dependency, so
// host/test_intra_chain.cpp compiles them with g++ and the expansion kernel of intra_chain.hip uses the same text.
//   intraChainPred      prediction p of the two job tables: its block and its offset (0 .. nIntra - 1 regular, then MIP)
//   intraChainTuOk      what a vtmhip_intra_tu_job must satisfy on a W x H block
//   intraChainExpand    the job as a vtmhip_tu_job of the fused chain: the residual of its prediction at stride W, shape and bit depth from the block
//   intraChainScan      the host pass over all four tables: every entry is checked (with intraBlockOk / intraModeOk / mipBlockOk / mipJobOk: the rules the prediction
//                       kernels skip by), and the launch plan falls out of the same walk (chain_rules.hpp's ChainShapes over the TU jobs)
//   intraChainExpandAll the expansion of a whole checked TU table, for both make-jobs entries (lfnst_rules.hpp calls it too)
// A table with one malformed entry is rejected whole: the chain kernels trust their jobs.
#pragma once
#include "chain_rules.hpp"
#include "intra_rules.hpp"
#include "mip_rules.hpp"

#if defined( __HIPCC__ )
#define ICHAIN_HD __host__ __device__ inline
#else
#define ICHAIN_HD inline
#endif

struct IntraChainPlan
{
  int         maxBlockArea;   // over the block table: decides the lanes a prediction job gets
  ChainShapes tu;             // over the TU jobs
};

ICHAIN_HD void intraChainPred( const vtmhip_intra_job *intraJobs, int nIntra, const vtmhip_mip_job *mipJobs, int p, int &block, int64_t &predOff )
{
  if( p < nIntra ) { block = intraJobs[p].block; predOff = intraJobs[p].predOff; }
  else { block = mipJobs[p - nIntra].block; predOff = mipJobs[p - nIntra].predOff; }
}

ICHAIN_HD bool intraChainTrOk( int typeHor, int typeVer, int w, int h )
{
  if( typeHor == VTMHIP_TRSKIP || typeVer == VTMHIP_TRSKIP ) return typeHor == typeVer && w <= 32 && h <= 32;
  if( typeHor > VTMHIP_DST7 || typeVer > VTMHIP_DST7 ) return false;
  return ( typeHor == VTMHIP_DCT2 || w <= 32 ) && ( typeVer == VTMHIP_DCT2 || h <= 32 );   // DCT8 / DST7 matrices end at 32
}

ICHAIN_HD bool intraChainTuOk( const vtmhip_intra_tu_job &t, int w, int h )
{
  return chainQpOk( t.qpPer, t.qpRem ) && t.reserved == 0 && t.pad == 0 && intraChainTrOk( t.typeHor, t.typeVer, w, h );
}

ICHAIN_HD void intraChainExpand( const vtmhip_intra_tu_job &t, const vtmhip_intra_block &b, int64_t predOff, vtmhip_tu_job &out )
{
  out.resiOff    = predOff;
  out.outOff     = t.outOff;
  out.resiStride = b.width;
  out.width = b.width; out.height = b.height;
  out.qpPer = t.qpPer; out.qpRem = t.qpRem;
  out.typeHor = t.typeHor; out.typeVer = t.typeVer;
  out.bitDepth = b.bitDepth; out.isIRAP = t.isIRAP;
  out.pad = 0; out.chromaAdj = 0;
}

// false: an entry the prediction entries would skip or the chain must not see
inline bool intraChainScan( const vtmhip_intra_block *blocks, int numBlocks, const vtmhip_intra_job *intraJobs, int nIntra, const vtmhip_mip_job *mipJobs, int nMip,
                            const vtmhip_intra_tu_job *tuJobs, int nTu, IntraChainPlan &plan )
{
  plan.maxBlockArea = 0;
  plan.tu.begin( nTu );
  for( int i = 0; i < numBlocks; i++ )
  {
    const vtmhip_intra_block &b = blocks[i];
    if( !intraBlockOk( b.width, b.height, b.bitDepth, b.multiRefIdx ) || b.reserved[0] || b.reserved[1] ) return false;
    if( b.width * b.height > plan.maxBlockArea ) plan.maxBlockArea = b.width * b.height;
  }
  for( int i = 0; i < nIntra; i++ )
  {
    const vtmhip_intra_job &j = intraJobs[i];
    if( j.block < 0 || j.block >= numBlocks || !intraModeOk( j.mode, blocks[j.block].multiRefIdx ) || j.reserved[0] || j.reserved[1] || j.reserved[2] ) return false;
  }
  for( int i = 0; i < nMip; i++ )
  {
    const vtmhip_mip_job &j = mipJobs[i];
    if( j.block < 0 || j.block >= numBlocks || j.reserved[0] || j.reserved[1] ) return false;
    const vtmhip_intra_block &b = blocks[j.block];
    if( !mipBlockOk( b.width, b.height, b.bitDepth, b.multiRefIdx ) || !mipJobOk( mipShape( b.width, b.height ), j.mode, j.transposed ) ) return false;
  }
  for( int i = 0; i < nTu; i++ )
  {
    const vtmhip_intra_tu_job &t = tuJobs[i];
    if( t.pred < 0 || t.pred >= nIntra + nMip ) return false;
    int     blk;
    int64_t predOff;
    intraChainPred( intraJobs, nIntra, mipJobs, t.pred, blk, predOff );
    const int w = blocks[blk].width, h = blocks[blk].height;
    if( !intraChainTuOk( t, w, h ) ) return false;
    plan.tu.add( i, w, h, t.typeHor );
  }
  return true;
}

// out[i] = TU job i as the chain sees it; the tables have passed intraChainScan
inline void intraChainExpandAll( const vtmhip_intra_block *blocks, const vtmhip_intra_job *intraJobs, int nIntra, const vtmhip_mip_job *mipJobs,
                                 const vtmhip_intra_tu_job *tuJobs, int nTu, vtmhip_tu_job *out )
{
  for( int i = 0; i < nTu; i++ )
  {
    int     blk;
    int64_t predOff;
    intraChainPred( intraJobs, nIntra, mipJobs, tuJobs[i].pred, blk, predOff );
    intraChainExpand( tuJobs[i], blocks[blk], predOff, out[i] );
  }
}

// vtmhip_intra_chain_make_tu_jobs without its NULL checks: out[i] = TU job i as the chain sees it; nothing is written when a table is rejected
inline bool intraChainMakeTuJobs( const vtmhip_intra_block *blocks, int numBlocks, const vtmhip_intra_job *intraJobs, int nIntra, const vtmhip_mip_job *mipJobs, int nMip,
                                  const vtmhip_intra_tu_job *tuJobs, int nTu, vtmhip_tu_job *out, IntraChainPlan &plan )
{
  if( !intraChainScan( blocks, numBlocks, intraJobs, nIntra, mipJobs, nMip, tuJobs, nTu, plan ) ) return false;
  intraChainExpandAll( blocks, intraJobs, nIntra, mipJobs, tuJobs, nTu, out );
  return true;
}
