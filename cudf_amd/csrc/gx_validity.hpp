// gx_validity.hpp -- the one place for how a value kernel reads and writes the words of an Arrow validity bitmap (LSB-first bits in
// uint32 words, 1 = valid; cudf/utilities/bit.hpp:47-61).  What gx_rows.hpp is to the key kernels' element rules.
//
// Part (a) is plain word arithmetic without a HIP include: tests/cpp/gx_validity_tests.cpp compiles it with g++ and checks it bit by
// bit on arrays that end at the last word a call may read.  What every reader below keeps:
//   * only words that hold a requested bit are read -- none in front of the first bit, none behind the last;
//   * no shift by the operand's full width (32 or 64) is ever evaluated;
//   * bits at and above the requested count are 0 in the result.
// Part (b), the device helpers, needs the wave primitives: under hipcc this header is included through gx_common.hpp.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define GX_HD __host__ __device__
#else
#define GX_HD
#endif
#define GX_HD_INLINE GX_HD inline __attribute__((always_inline))

namespace gx {

GX_HD_INLINE bool bit_is_set(const uint32_t* mask, int64_t i) { return (mask[i >> 5] >> (i & 31)) & 1u; }
GX_HD_INLINE bool row_valid(const uint32_t* mask, int64_t i) { return mask == nullptr || bit_is_set(mask, i); }

// the low cnt bits set: cnt in 0..32 / 0..64
GX_HD_INLINE uint32_t low_mask32(int cnt) { return cnt >= 32 ? 0xFFFFFFFFu : ((1u << cnt) - 1u); }
GX_HD_INLINE uint64_t low_mask64(int cnt) { return cnt >= 64 ? ~0ull : ((1ull << cnt) - 1ull); }

// the bits of word w (bits [32 w, 32 w + 32)) that lie in [begin_bit, end_bit)
GX_HD_INLINE uint32_t word_range_mask(int64_t w, int64_t begin_bit, int64_t end_bit)
{
  const int64_t lo = w * 32, hi = lo + 32;
  if (hi <= begin_bit || lo >= end_bit) return 0u;
  uint32_t m = 0xFFFFFFFFu;
  if (begin_bit > lo) m &= 0xFFFFFFFFu << (begin_bit - lo);
  if (end_bit < hi) m &= 0xFFFFFFFFu >> (hi - end_bit);
  return m;
}

// cnt (1..32) bits of `m` from bit `bit` on, in the low bits of the result: the second word is read only when the run crosses into it
GX_HD_INLINE uint32_t bits_from(const uint32_t* __restrict__ m, int64_t bit, int cnt)
{
  const int64_t w = bit >> 5;
  const int sh    = (int)(bit & 31);
  uint64_t two    = m[w];
  if (sh + cnt > 32) two |= (uint64_t)m[w + 1] << 32;
  return (uint32_t)(two >> sh) & low_mask32(cnt);
}

// the bits [bit, end_bit) of `m` (1..64 of them) in the low bits of the result: one to three words, the last the word of end_bit - 1.
// A wave whose 64 rows start at `bit` calls it with a wave-uniform address, so the loads are scalar loads.
GX_HD_INLINE uint64_t bits_from64(const uint32_t* __restrict__ m, int64_t bit, int64_t end_bit)
{
  const int64_t w    = bit >> 5;
  const int sh       = (int)(bit & 31);
  const int64_t last = (end_bit - 1) >> 5;
  uint64_t lo        = m[w];
  if (w + 1 <= last) lo |= (uint64_t)m[w + 1] << 32;
  if (sh != 0) {
    uint64_t hi = 0;
    if (w + 2 <= last) hi = m[w + 2];
    lo = (lo >> sh) | (hi << (64 - sh));
  }
  return lo & low_mask64((int)(end_bit - bit));
}

#ifdef __HIPCC__
// ---------------------------------------------------------------- device: writing the validity of a wave's 64 rows
// A wave holds 64 consecutive rows from first_row (a multiple of 64) on; bit l of `b` is the validity of lane l's row, 0 for a row at
// or behind n.  Lane 0 writes word first_row >> 5 and the word behind it, each only when it is one of the (n + 31) >> 5 words of
// the bitmap, so bits at and above n of the last word are 0 and nothing behind it is touched.
__device__ __forceinline__ void store_wave_words(uint32_t* __restrict__ out_valid, int64_t first_row, int64_t n, uint64_t b)
{
  if (lane_id() == 0) {
    const int64_t w = first_row >> 5, nwords = (n + 31) >> 5;
    if (w < nwords) out_valid[w] = (uint32_t)b;
    if (w + 1 < nwords) out_valid[w + 1] = (uint32_t)(b >> 32);
  }
}
// the same from `ok`, the validity of this lane's row; returns the ballot.  Every lane of the wave must call it.
__device__ __forceinline__ uint64_t store_wave_validity(uint32_t* __restrict__ out_valid, int64_t first_row, int64_t n, bool ok)
{
  const uint64_t b = ballot(ok);
  store_wave_words(out_valid, first_row, n, b);
  return b;
}

// ---------------------------------------------------------------- device: the null count of a workgroup
// The kernel declares one __shared__ word `s` (unsigned int where a workgroup's rows fit, else unsigned long long).  tally_begin zeroes
// it and ends in a barrier; tally_end takes from lane 0 of every wave that wave's count (one LDS atomic per wave with a non-zero
// count), meets in a barrier and adds the workgroup's count to *null_count (one global atomic per workgroup with a non-zero count;
// none when null_count is NULL).  Both are called by every thread of the workgroup.
template <typename C>
__device__ __forceinline__ void tally_begin(C* s)
{
  if (threadIdx.x == 0) *s = 0;
  __syncthreads();
}
template <typename C>
__device__ __forceinline__ void tally_end(C* s, C wave_count, unsigned long long* __restrict__ null_count)
{
  if (lane_id() == 0 && wave_count) atomicAdd(s, wave_count);
  __syncthreads();
  if (threadIdx.x == 0 && *s && null_count) atomicAdd(null_count, (unsigned long long)*s);
}

// ---------------------------------------------------------------- device: a column or a scalar as the source of values
// A column (is_scalar == 0: data[i], validity bit begin_bit + i of `valid`, NULL = no nulls) or a scalar (data[0]; valid == NULL;
// its validity is the device byte scalar_valid, NULL = valid).
struct ValueSrc {
  const void* data;
  const uint32_t* valid;
  int64_t begin_bit;
  const uint8_t* scalar_valid;
  int is_scalar;
  // what every row without a bitmap has: read once per thread, in front of the row loop, and handed to bits64
  __device__ __forceinline__ bool scalar_ok() const { return !(is_scalar && scalar_valid) || *scalar_valid != 0; }
  // validity of the rows [row0, end) of a wave (1..64 rows; row0 wave-uniform: bits_from64)
  __device__ __forceinline__ uint64_t bits64(int64_t row0, int64_t end, bool ok) const
  {
    return valid ? bits_from64(valid, begin_bit + row0, begin_bit + end) : (ok ? low_mask64((int)(end - row0)) : 0ull);
  }
};
#endif  // __HIPCC__

}  // namespace gx
