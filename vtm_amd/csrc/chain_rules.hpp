// chain_rules.hpp -- what the table rules of the level entries share (intra_chain_rules.hpp, intra_chroma_chain_rules.hpp, lfnst_rules.hpp): plain integer
// code without a HIP dependency, compiled by the host programs of all three with g++.
//   chainQpOk      the quantiser fields every job table carries
//   ChainShapes    the walk over one table of TU jobs: the largest sides and area, and whether the table still has one size and real transforms
#pragma once
#include "../../include/vtmhip.h"

#if defined( __HIPCC__ )
#define CHAIN_HD __host__ __device__ inline
#else
#define CHAIN_HD inline
#endif

CHAIN_HD bool chainQpOk( int qpPer, int qpRem ) { return qpRem >= 0 && qpRem <= 5 && qpPer >= 0; }

struct ChainShapes
{
  int maxWidth, maxHeight, maxArea;   // over the jobs (0 without any)
  int uniform;                        // every job has one size and no transform skip: what the chains' uniformSize asks
  void begin( int n ) { maxWidth = maxHeight = maxArea = 0; uniform = n > 0; }
  void add( int i, int w, int h, int typeHor )   // job i of the table
  {
    if( i && ( w != maxWidth || h != maxHeight ) ) uniform = 0;   // before the first difference the maxima are the one size
    if( typeHor == VTMHIP_TRSKIP ) uniform = 0;
    if( w > maxWidth ) maxWidth = w;
    if( h > maxHeight ) maxHeight = h;
    if( w * h > maxArea ) maxArea = w * h;
  }
};
