// What does the ACCESS PATTERN of k_hf_sample cost, with nothing else in the kernel?  One wave reads one 512-byte chunk (64 keys) at
// every `step` keys of an n-key column and ORs it into a register; workgroups of four waves take contiguous runs of chunks, 16 loads in
// flight per wave (the sample's loop, gx_sort.hip).  No transform, no histogram, no atomics: one store per workgroup.
//   step 2048   the sample at n >= 2^27: 512 B of every 16 KiB
//   step 2112   the same number of chunks 16.5 KiB apart (not a power of two: another spread over the memory channels)
//   step   64   the same number of chunks back to back (a dense read of the same bytes: what "its bytes cost" would be)
// Every step is timed WARM (the same launch again, nothing in between: at 1e9 keys the 250 MB it reads fit the 256 MiB Infinity Cache,
// so this is a cache-hit figure) and COLD (2 GiB of an unrelated buffer streamed through the memory system between two timed
// launches: what the sort sees, where 48 GB move between two samples).
// usage: xp_strided_read [log2 n, default 1e9 keys]
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#define CHECK(x)                                                                  \
  do {                                                                            \
    hipError_t e_ = (x);                                                          \
    if (e_ != hipSuccess) {                                                       \
      printf("%s failed: %s\n", #x, hipGetErrorString(e_));                       \
      return 1;                                                                   \
    }                                                                             \
  } while (0)

__global__ void __launch_bounds__(256) k_read(const uint64_t* __restrict__ in, int64_t n, int64_t step, int64_t nchunks, uint64_t* __restrict__ out)
{
  constexpr int U      = 16;
  const int lane       = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t per    = (nchunks + gridDim.x - 1) / gridDim.x;
  const int64_t c_lo   = (int64_t)blockIdx.x * per;
  const int64_t c_hi   = c_lo + per < nchunks ? c_lo + per : nchunks;
  uint64_t acc = 0;
  for (int64_t c0 = c_lo + wave; c0 < c_hi; c0 += 4 * U) {
    uint64_t raw[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t row = (c0 + 4 * u) * step + lane;
      raw[u]            = (c0 + 4 * u < c_hi && row < n) ? in[row] : 0ull;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) acc |= raw[u];
  }
  __shared__ uint64_t s[256];
  s[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t o = 0;
    for (int i = 0; i < 256; ++i) o |= s[i];
    out[blockIdx.x] = o;
  }
}

// the cold mode's flush: reads `n16` 16-byte words of an unrelated buffer, one store per workgroup
__global__ void __launch_bounds__(256) k_flush(const uint4* __restrict__ buf, size_t n16, uint32_t* __restrict__ out)
{
  uint32_t acc = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (size_t)gridDim.x * 256) {
    const uint4 q = buf[i];
    acc |= q.x | q.y | q.z | q.w;
  }
  if (acc == 0xFFFFFFFFu) out[blockIdx.x] = acc;  // (never: the buffer holds 0x11 bytes; keeps the loads alive)
}

int main(int argc, char** argv)
{
  const int64_t n = argc > 1 ? (int64_t)1 << atoi(argv[1]) : 1000000000ll;
  uint64_t *in = nullptr, *out = nullptr;
  const int grid = 2048;
  CHECK(hipMalloc(&in, (size_t)n * 8));
  CHECK(hipMalloc(&out, (size_t)grid * 8));
  CHECK(hipMemset(in, 0x5A, (size_t)n * 8));
  const size_t flush_bytes = (size_t)2 << 30;  // 8 x the Infinity Cache
  uint4* flush             = nullptr;
  uint32_t* fout           = nullptr;
  CHECK(hipMalloc(&flush, flush_bytes));
  CHECK(hipMalloc(&fout, 4096 * 4));
  CHECK(hipMemset(flush, 0x11, flush_bytes));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  const int64_t nchunks = (n + 2047) / 2048;  // the sample's chunk count at stride 32
  const int64_t steps[3] = {2048, 2112, 64};
  for (int v = 0; v < 3; ++v) {
    const int64_t step = steps[v];
    int64_t nc         = nchunks;
    if ((nc - 1) * step >= n) nc = (n - 1) / step + 1;  // (step 2112: the last chunks would start past the column)
    for (int cold = 0; cold < 2; ++cold) {
      float best = 1e30f, worst = 0.f;
      for (int rep = 0; rep < 7; ++rep) {
        if (cold) hipLaunchKernelGGL(k_flush, dim3(4096), dim3(256), 0, 0, flush, flush_bytes / 16, fout);
        CHECK(hipEventRecord(e0, 0));
        hipLaunchKernelGGL(k_read, dim3(grid), dim3(256), 0, 0, in, n, step, nc, out);
        CHECK(hipEventRecord(e1, 0));
        CHECK(hipEventSynchronize(e1));
        float ms = 0.f;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if (rep >= 2) {
          best  = ms < best ? ms : best;
          worst = ms > worst ? ms : worst;
        }
      }
      CHECK(hipGetLastError());
      const double bytes = (double)nc * 512.0;
      printf("%s n %lld keys, %lld chunks of 512 B every %lld keys (%.1f KiB): %.1f MB  min %.1f us  max %.1f us (5 launches)  %.2f TB/s\n", cold ? "COLD" : "warm",
             (long long)n, (long long)nc, (long long)step, step * 8 / 1024.0, bytes / 1e6, best * 1e3, worst * 1e3, bytes / (best * 1e-3) / 1e12);
    }
  }
  CHECK(hipFree(flush));
  CHECK(hipFree(fout));
  CHECK(hipFree(in));
  CHECK(hipFree(out));
  printf("ok\n");
  return 0;
}
