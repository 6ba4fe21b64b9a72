// test_isp.cpp -- the ISP rules of vtm_amd/csrc/isp_rules.hpp and the host chain of isp_host.hpp (both HIP-free) as a stand-alone program under AddressSanitizer and
// UBSan (tests/test_isp_cpp.py builds and runs it).  Every table and buffer sits in a heap array of exactly its length, so a read or write past one is a report; every
// index a prediction reads a line at goes through INTRA_LINE_CHECK, and every read of the line update (the CU's side line, the reconstruction) through
// ISP_READ_CHECK; either is counted when it lies outside its array (the lines of a region end at cuW + regW and cuH + regH, the CU's at 2W and 2H -- top and left
// share one allocation, as a block's lines do, so the sanitizer alone would not see a read of one past its end into the other).  The full chain runs on 4x8,
// 8x4, 4x16, 16x4, 8x8 and 16x16 with every mode, both splits, both availability branches and three bit depths; what it leaves is checked for what can be said without a second implementation: the reconstruction inside the sample range, the reported SSE equal to the one recomputed
// from the outputs, zero levels exactly where absSum says so, and malformed tables rejected with nothing written.
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>

static long g_lineReads = 0, g_updateReads = 0, g_lineOutside = 0;
#define INTRA_LINE_CHECK( idx, last ) do { g_lineReads++; if( ( idx ) < 0 || ( idx ) > ( last ) ) g_lineOutside++; } while( 0 )
#define ISP_READ_CHECK( idx, last ) do { g_updateReads++; if( ( idx ) < 0 || ( idx ) > ( last ) ) g_lineOutside++; } while( 0 )
#include "../vtm_amd/csrc/isp_host.hpp"

static int g_failures = 0;
#define EXPECT( cond ) do { if( !( cond ) ) { g_failures++; if( g_failures < 20 ) printf( "FAIL %s:%d %s\n", __FILE__, __LINE__, #cond ); } } while( 0 )

template<class T> static std::unique_ptr<T[]> heap( size_t n, T fill ) { std::unique_ptr<T[]> p( new T[n] ); for( size_t i = 0; i < n; i++ ) p[i] = fill; return p; }

static void run_shape( int w, int h, int bd, std::mt19937 &rng, long &jobsRun )
{
  const int maxVal = ( 1 << bd ) - 1, nRef = 2 * w + 1 + 2 * h + 1, n = 67 * 2 * 2;
  auto ref = heap<int16_t>( nRef, 0 ), org = heap<int16_t>( ( size_t ) w * h, 0 );
  for( int i = 0; i < nRef; i++ ) ref[i] = ( int16_t ) ( rng() % ( maxVal + 1 ) );
  ref[2 * w + 1] = ref[0];   // one corner
  for( int i = 0; i < w * h; i++ ) org[i] = ( int16_t ) ( rng() % ( maxVal + 1 ) );
  auto blocks = heap<vtmhip_intra_block>( 1, vtmhip_intra_block() );
  blocks[0].refOff = 0; blocks[0].orgOff = 0; blocks[0].orgStride = w; blocks[0].width = ( int16_t ) w; blocks[0].height = ( int16_t ) h; blocks[0].bitDepth = ( uint8_t ) bd;
  auto jobs = heap<vtmhip_isp_job>( n, vtmhip_isp_job() );
  for( int i = 0; i < n; i++ )
  {
    const int qp = 10 + ( int ) ( rng() % 42 ) + 6 * ( bd - 8 );
    jobs[i].predOff = jobs[i].outOff = ( int64_t ) i * w * h;
    jobs[i].block = 0; jobs[i].qpPer = ( int16_t ) ( qp / 6 ); jobs[i].qpRem = ( int16_t ) ( qp % 6 );
    jobs[i].mode = ( uint8_t ) ( i % 67 ); jobs[i].split = ( uint8_t ) ( 1 + ( i / 67 ) % 2 ); jobs[i].sideAvail = ( uint8_t ) ( ( i / 134 ) % 2 ); jobs[i].isIRAP = ( uint8_t ) ( i & 1 );
  }
  IspPlan plan;
  EXPECT( ispScan( blocks.get(), 1, jobs.get(), n, plan ) );
  EXPECT( plan.maxArea == w * h && plan.jobInts > 0 );
  const size_t total = ( size_t ) n * w * h;
  auto pred = heap<int16_t>( total, -1 ), reco = heap<int16_t>( total, -1 );
  auto levels = heap<int32_t>( total, 0x5a5a5a5a );
  auto results = heap<vtmhip_isp_result>( n, vtmhip_isp_result() );
  for( int i = 0; i < n; i++ ) isp_host::chainJob( ref.get(), org.get(), blocks[0], jobs[i], pred.get(), levels.get(), reco.get(), results[i] );
  jobsRun += n;
  for( int i = 0; i < n; i++ )
  {
    IspGeom g;
    ispGeometry( w, h, jobs[i].split, g );
    EXPECT( results[i].numParts == g.numParts && g.numParts * g.partW * g.partH == w * h );
    const int16_t *rc = reco.get() + ( size_t ) i * w * h, *pr = pred.get() + ( size_t ) i * w * h;
    const int32_t *lv = levels.get() + ( size_t ) i * w * h;
    for( int k = 0; k < g.numParts; k++ )
    {
      int px, py;
      ispPartRect( g, jobs[i].split, k, px, py );
      uint64_t sse = 0;
      long     sumLevels = 0;
      for( int y = 0; y < g.partH; y++ )
        for( int x = 0; x < g.partW; x++ )
        {
          const int at = ( py + y ) * w + px + x, d = org[at] - rc[at];
          EXPECT( rc[at] >= 0 && rc[at] <= maxVal && pr[at] >= 0 && pr[at] <= maxVal );
          sse += ( uint64_t ) ( d * d );
          sumLevels += std::abs( lv[k * g.partW * g.partH + y * g.partW + x] );
          if( results[i].absSum[k] == 0 ) EXPECT( rc[at] == pr[at] );   // nothing coded: the reconstruction is the prediction
        }
      EXPECT( sse == results[i].sse[k] );
      EXPECT( sumLevels == results[i].absSum[k] );   // no level reaches the 16-bit clip at these sizes
    }
    for( int k = g.numParts; k < ISP_MAX_PARTS; k++ ) EXPECT( results[i].sse[k] == 0 && results[i].absSum[k] == 0 && results[i].sumAbs[k] == 0 );
  }
  // without the optional outputs: the same reconstruction
  auto reco2 = heap<int16_t>( ( size_t ) w * h, -1 );
  vtmhip_isp_job j0 = jobs[5];
  j0.outOff = 0;
  vtmhip_isp_result r0;
  isp_host::chainJob( ref.get(), org.get(), blocks[0], j0, nullptr, nullptr, reco2.get(), r0 );
  EXPECT( memcmp( reco2.get(), reco.get() + ( size_t ) 5 * w * h, sizeof( int16_t ) * w * h ) == 0 );
}

static void rejected()
{
  auto blocks = heap<vtmhip_intra_block>( 2, vtmhip_intra_block() );
  auto jobs   = heap<vtmhip_isp_job>( 2, vtmhip_isp_job() );
  auto reset = [&]() {
    for( int i = 0; i < 2; i++ )
    {
      blocks[i] = vtmhip_intra_block(); blocks[i].width = 8; blocks[i].height = ( int16_t ) ( 8 << i ); blocks[i].bitDepth = 10;
      jobs[i] = vtmhip_isp_job(); jobs[i].block = i; jobs[i].split = ( uint8_t ) ( 1 + i ); jobs[i].mode = 34; jobs[i].qpPer = 5; jobs[i].qpRem = 2;
    }
  };
  IspPlan plan;
  reset(); EXPECT( ispScan( blocks.get(), 2, jobs.get(), 2, plan ) );
  reset(); blocks[0].width = 4; blocks[0].height = 4; EXPECT( !ispScan( blocks.get(), 2, jobs.get(), 2, plan ) );
  reset(); blocks[1].width = 128; EXPECT( !ispScan( blocks.get(), 2, jobs.get(), 2, plan ) );
  reset(); blocks[1].multiRefIdx = 1; EXPECT( !ispScan( blocks.get(), 2, jobs.get(), 2, plan ) );
  reset(); blocks[0].bitDepth = 13; EXPECT( !ispScan( blocks.get(), 2, jobs.get(), 2, plan ) );
  reset(); blocks[0].reserved[1] = 1; EXPECT( !ispScan( blocks.get(), 2, jobs.get(), 2, plan ) );
  reset(); jobs[0].mode = 67; EXPECT( !ispScan( blocks.get(), 2, jobs.get(), 2, plan ) );
  reset(); jobs[1].split = 0; EXPECT( !ispScan( blocks.get(), 2, jobs.get(), 2, plan ) );
  reset(); jobs[1].split = 3; EXPECT( !ispScan( blocks.get(), 2, jobs.get(), 2, plan ) );
  reset(); jobs[0].qpRem = 6; EXPECT( !ispScan( blocks.get(), 2, jobs.get(), 2, plan ) );
  reset(); jobs[0].qpPer = -1; EXPECT( !ispScan( blocks.get(), 2, jobs.get(), 2, plan ) );
  reset(); jobs[1].reserved[3] = 1; EXPECT( !ispScan( blocks.get(), 2, jobs.get(), 2, plan ) );
  reset(); jobs[1].block = 2; EXPECT( !ispScan( blocks.get(), 2, jobs.get(), 2, plan ) );
  reset(); jobs[0].block = -1; EXPECT( !ispScan( blocks.get(), 2, jobs.get(), 2, plan ) );
  reset(); jobs[0].sideAvail = 2; EXPECT( !ispScan( blocks.get(), 2, jobs.get(), 2, plan ) );
}

int main()
{
  std::mt19937 rng( 12345 );
  const int    shapes[6][2] = { { 4, 8 }, { 8, 4 }, { 4, 16 }, { 16, 4 }, { 8, 8 }, { 16, 16 } };
  long         jobsRun = 0;
  for( int s = 0; s < 6; s++ )
    for( int bd = 8; bd <= 12; bd += 2 ) run_shape( shapes[s][0], shapes[s][1], bd, rng, jobsRun );
  rejected();
  printf( "%ld jobs, %d failures, %ld line reads, %ld reads of the line update, %ld outside their line\n", jobsRun, g_failures, g_lineReads, g_updateReads, g_lineOutside );
  return g_failures || g_lineOutside ? 1 : 0;
}
