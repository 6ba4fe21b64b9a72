// intra_lane_rule.hpp -- the lane rule of the intra kernels that work from a vtmhip_intra_block table, without the kernel that evaluates it on the device
// (intra_lanes.hpp): a job gets 16, 64 or 256 lanes by the largest well-formed block of the table, and a workgroup takes 16 / 8 / 4 consecutive jobs.  The
// prediction bodies (intra_body.hpp, mip_body.hpp) and intra_chain.hip, whose entry knows the largest block on the host, need no more than this.
#pragma once

namespace
{

constexpr int INTRA_MAX_AREA = 4096;

__host__ __device__ inline int intra_lanes( int maxArea ) { return maxArea < 16 || maxArea > INTRA_MAX_AREA ? 0 : maxArea <= 64 ? 16 : maxArea <= 1024 ? 64 : 256; }
__host__ __device__ inline int intra_chunk( int lanes ) { return lanes == 16 ? 16 : lanes == 64 ? 8 : 4; }
constexpr int INTRA_MIN_CHUNK = 4;

}   // namespace
