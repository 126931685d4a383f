// gx_compact.hpp -- what every SELECTOR of the ordered stream compaction shares (gx_compact.hip: mask / validity / NaN selectors and
// the scatters; gx_distinct.hip: the deduplicating selectors): the plan and its layout in the caller's scratch, the predicate
// select kernel, the scan of the chunk counts behind it, the prologue of an entry point.
#pragma once
#include "gx_rows.hpp"
#include "gx_scan.hpp"

namespace gx {
namespace compact {

constexpr int SEL_CHUNK = 4096;                 // rows per chunk (256 threads x 16 wave-rows of 64)
constexpr int SEL_WORDS = SEL_CHUNK / GX_WAVE;  // ballot words per chunk
using rows::MAX_KEYS;                           // key columns of one selection

GX_LOCAL inline std::atomic<int> g_stages{3};  // measurement hook (gx_knobs.h): bit 0 = the select kernel runs, bit 1 = the scan

struct Plan {
  uint64_t* bits;     // ceil(n / 64) + 1 words: bit (i & 63) of word i >> 6 = row i is kept
  long long* starts;  // nchunks + 1: selected rows before the chunk; [nchunks] = the total
  int64_t nchunks;
  size_t bytes;
};
static inline Plan carve(const void* tmp, int64_t n)
{
  Carver c(const_cast<void*>(tmp));
  Plan p;
  p.nchunks = n > 0 ? div_up(n, (int64_t)SEL_CHUNK) : 0;
  p.bits    = c.take<uint64_t>((size_t)(n > 0 ? div_up(n, (int64_t)GX_WAVE) : 0) + 1);
  p.starts  = c.take<long long>((size_t)p.nchunks + 1);
  p.bytes   = c.total();
  return p;
}

// one row per lane, any predicate: wave w takes wave-rows w, w + 4, ... of the chunk
template <typename Pred>
__global__ void __launch_bounds__(256) k_select_pred(Pred pred, int64_t n, uint64_t* __restrict__ bits,
                                                     long long* __restrict__ chunk_count)
{
  __shared__ unsigned int s_cnt;
  const unsigned lane = lane_id();
  const unsigned w    = threadIdx.x / GX_WAVE;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * SEL_CHUNK;
  unsigned int mine  = 0;
  for (int k = 0; k < SEL_CHUNK / 256; ++k) {
    const int64_t row0 = base + (int64_t)(k * 4 + w) * GX_WAVE;
    const int64_t i    = row0 + lane;
    const bool sel     = i < n && pred(i);
    const uint64_t b   = ballot(sel);
    if (lane == 0 && row0 < n) {
      bits[row0 >> 6] = b;
      mine += (unsigned int)__builtin_popcountll(b);
    }
  }
  if (lane == 0 && mine) atomicAdd(&s_cnt, mine);
  __syncthreads();
  if (threadIdx.x == 0) chunk_count[blockIdx.x] = s_cnt;
}

static __global__ void k_store_total(const long long* __restrict__ starts, int64_t nchunks, long long* __restrict__ count_out)
{
  if (threadIdx.x == 0 && blockIdx.x == 0) *count_out = starts[nchunks];
}

// select kernel (whichever `launch_select` issues), scan of the chunk counts, the total to *count_dev
template <typename LaunchSelect>
int run_stages(LaunchSelect&& launch_select, const Plan& p, int64_t* count_dev, hipStream_t s)
{
  const int stages = g_stages.load(std::memory_order_relaxed);
  if (stages & 1) launch_select();
  if (stages & 2) {
    hipLaunchKernelGGL((scan::k_partials_scan<long long, SumOp>), dim3(1), dim3(1024), 0, s, p.starts, p.nchunks, 0ll, SumOp(),
                       (const int*)nullptr);
    if (count_dev) hipLaunchKernelGGL(k_store_total, dim3(1), dim3(64), 0, s, p.starts, p.nchunks, reinterpret_cast<long long*>(count_dev));
  }
  GX_LAUNCH_CHECK();
  return 0;
}
template <typename Pred>
int select_launch(const Pred& pred, int64_t n, const Plan& p, int64_t* count_dev, hipStream_t s)
{
  return run_stages([&] { hipLaunchKernelGGL((k_select_pred<Pred>), dim3((unsigned)p.nchunks), dim3(256), 0, s, pred, n, p.bits, p.starts); },
                    p, count_dev, s);
}

static inline int check_rows(int64_t n) { return (n < 0 || n > 0x7FFFFFFFll) ? GX_EINVAL : 0; }

}  // namespace compact
}  // namespace gx
