// gx_copying.hip -- the row-movement kernels behind <cudf/copying.hpp> and <cudf/concatenate.hpp>: a fused concatenate of any
// number of columns (data + validity + null count in one launch), scatter (the mirror of k_gather, gx_gather.hip) and
// copy_if_else (an element-wise select).  reference: cpp/src/copying/concatenate.cu (fused_concatenate_kernel, concatenate_masks),
// cpp/include/cudf/detail/scatter.cuh, cpp/include/cudf/detail/copy_if_else.cuh.  All three are HBM-bound: streaming reads and
// writes (concatenate, copy_if_else), a streaming read plus a random write (scatter).  Validity bitmaps are Arrow bitmaps read
// from a begin bit on, so sliced views need no re-based copy.
#include "gx_common.hpp"

namespace gx {

constexpr int COPY_BT = 256;

// ---------------------------------------------------------------- concatenate
// One workgroup per tile of CONCAT_TILE consecutive OUTPUT rows.  The tile is a multiple of 32 rows, so a tile owns whole
// validity words: no two workgroups ever touch one word and nothing is merged with atomics.
constexpr int CONCAT_TILE      = 4096;
constexpr int CONCAT_ROW_PATH  = 16;  // a tile fed by more inputs than this copies row by row (each row searches its input)
constexpr int CONCAT_DESC_BATCH = 64;

// the input descriptors in device memory: start[k] = first output row of input k, start[ninputs] = all rows
struct ConcatDesc {
  const long long* start;
  const char* const* src;
  const uint32_t* const* valid;  // NULL entry = no nulls
  const long long* bbit;         // begin bit of valid[k]
  int ninputs;
};

// the descriptors travel as kernel arguments, CONCAT_DESC_BATCH at a time: no host array is read after the call returns and
// nothing waits for the stream
struct ConcatDescBatch {
  long long start[CONCAT_DESC_BATCH];
  const char* src[CONCAT_DESC_BATCH];
  const uint32_t* valid[CONCAT_DESC_BATCH];
  long long bbit[CONCAT_DESC_BATCH];
  long long total;  // written behind the last entry when `last`
  int base, count, last;
};

__global__ void __launch_bounds__(CONCAT_DESC_BATCH) k_concat_put_desc(ConcatDescBatch b, long long* start, const char** src,
                                                                       const uint32_t** valid, long long* bbit)
{
  const int j = threadIdx.x;
  if (j < b.count) {
    start[b.base + j] = b.start[j];
    src[b.base + j]   = b.src[j];
    valid[b.base + j] = b.valid[j];
    bbit[b.base + j]  = b.bbit[j];
  }
  if (j == 0 && b.last) start[b.base + b.count] = b.total;
}

// the input that holds output row r (r < start[ninputs]), searched in [lo, hi): the LAST k with start[k] <= r, so that inputs
// without rows in front of it are skipped and start[k + 1] > r
__device__ __forceinline__ int concat_find(const long long* __restrict__ start, int lo, int hi, long long r)
{
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (start[mid] <= r) lo = mid; else hi = mid;
  }
  return lo;
}

// The validity word of output rows [r0, r1) (r0 a multiple of 32, r1 - r0 <= 32) composed from every input that has rows
// in it -- up to 32 of them, with any number of inputs without rows in between.  Bits from r1 - r0 on are 0.
__device__ __forceinline__ uint32_t concat_word(const ConcatDesc& d, long long r0, long long r1)
{
  int k         = concat_find(d.start, 0, d.ninputs, r0);
  uint32_t word = 0;
  long long r   = r0;
  while (r < r1) {  // r < start[ninputs], so k stays below ninputs
    const long long e = d.start[k + 1] < r1 ? d.start[k + 1] : r1;
    if (e > r) {
      const int cnt       = (int)(e - r);
      const uint32_t* m   = d.valid[k];
      const uint32_t bits = m ? bits_from(m, d.bbit[k] + (r - d.start[k]), cnt) : low_mask32(cnt);
      word |= bits << (int)(r - r0);
      r = e;
    }
    ++k;
  }
  return word;
}

// bytes [0, len) of s to d with accesses of V: bytes up to d's alignment, V's over the body, bytes behind it.  s and d agree
// in their address modulo sizeof(V) (the caller picks V that way).
template <typename V>
__device__ __forceinline__ void copy_span(char* d, const char* s, size_t len)
{
  const unsigned t = threadIdx.x;
  size_t head      = (size_t)((0 - reinterpret_cast<uintptr_t>(d)) & (sizeof(V) - 1));
  if (head > len) head = len;
  for (size_t i = t; i < head; i += COPY_BT) d[i] = s[i];
  const size_t nv = (len - head) / sizeof(V);
  const V* sv     = reinterpret_cast<const V*>(s + head);
  V* dv           = reinterpret_cast<V*>(d + head);
#pragma unroll 4
  for (size_t i = t; i < nv; i += COPY_BT) dv[i] = sv[i];
  for (size_t i = head + nv * sizeof(V) + t; i < len; i += COPY_BT) d[i] = s[i];
}

template <typename T>
__global__ void __launch_bounds__(COPY_BT) k_concat(ConcatDesc d, long long n, T* __restrict__ out, uint32_t* __restrict__ out_valid,
                                                    unsigned long long* __restrict__ null_count)
{
  __shared__ unsigned long long s_nulls;
  const long long t0 = (long long)blockIdx.x * CONCAT_TILE;
  const long long t1 = t0 + CONCAT_TILE < n ? t0 + CONCAT_TILE : n;
  const unsigned t   = threadIdx.x;

  // validity: thread j composes word j of the tile (CONCAT_TILE / 32 = 128 words, the first two waves)
  if (out_valid) {
    if (null_count) tally_begin(&s_nulls);
    const long long r0       = t0 + (long long)t * 32;
    unsigned long long nulls = 0;
    if (t < CONCAT_TILE / 32) {  // whole waves: CONCAT_TILE / 32 is a multiple of 64
      if (r0 < t1) {
        const long long r1  = r0 + 32 < t1 ? r0 + 32 : t1;
        const uint32_t word = concat_word(d, r0, r1);
        out_valid[r0 >> 5]  = word;
        nulls               = (unsigned long long)((r1 - r0) - __builtin_popcount(word));
      }
      if (null_count) nulls = wave_reduce(nulls, SumOp());
    }
    if (null_count) tally_end(&s_nulls, nulls, null_count);
  }

  // data (out == NULL: the validity alone, concatenate_masks)
  if (!out) return;
  const int k0 = concat_find(d.start, 0, d.ninputs, t0);
  const int k1 = concat_find(d.start, k0, d.ninputs, t1 - 1);
  if (k1 - k0 > CONCAT_ROW_PATH) {
    for (long long r = t0 + t; r < t1; r += COPY_BT) {
      const int k = concat_find(d.start, k0, k1 + 1, r);
      out[r]      = reinterpret_cast<const T*>(d.src[k])[r - d.start[k]];
    }
    return;
  }
  for (int k = k0; k <= k1; ++k) {
    const long long a = d.start[k] > t0 ? d.start[k] : t0;
    const long long b = d.start[k + 1] < t1 ? d.start[k + 1] : t1;
    if (b <= a) continue;
    const char* s    = d.src[k] + (size_t)(a - d.start[k]) * sizeof(T);
    char* dst        = reinterpret_cast<char*>(out + a);
    const size_t len = (size_t)(b - a) * sizeof(T);
    // the widest access the two addresses share: the destination offset of an input is (rows before it) * sizeof(T), so against
    // its source it is 16-byte aligned only by luck and, for 1- and 2-byte types, often not even 4-byte aligned
    const unsigned rel = (unsigned)((reinterpret_cast<uintptr_t>(s) ^ reinterpret_cast<uintptr_t>(dst)) & 15u);
    if (rel == 0) copy_span<uint4>(dst, s, len);
    else if ((rel & 7u) == 0) copy_span<uint2>(dst, s, len);
    else if ((rel & 3u) == 0) copy_span<uint32_t>(dst, s, len);
    else if ((rel & 1u) == 0) copy_span<uint16_t>(dst, s, len);
    else copy_span<uint8_t>(dst, s, len);
  }
}

template <typename T>
int concat_launch(const ConcatDesc& d, int64_t n, void* out, uint32_t* out_valid, int64_t* nulls, hipStream_t s)
{
  const int64_t tiles = div_up(n, CONCAT_TILE);
  hipLaunchKernelGGL((k_concat<T>), dim3((unsigned)tiles), dim3(COPY_BT), 0, s, d, (long long)n, static_cast<T*>(out), out_valid,
                     reinterpret_cast<unsigned long long*>(nulls));
  GX_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------- scatter
__device__ __forceinline__ int64_t wrap_row(int32_t m, int64_t rows) { return m < 0 ? (int64_t)m + rows : (int64_t)m; }

// bit `row` of `mask` set (ok) or cleared, atomically on its word; nothing is issued when the word read shows the bit in place
// already (the bit of a row changes only through writers of that row, so a stale read can only repeat a write)
__device__ __forceinline__ void put_bit(uint32_t* mask, int64_t row, bool ok)
{
  uint32_t* w      = mask + (row >> 5);
  const uint32_t b = 1u << (row & 31);
  const bool is    = (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & b) != 0;
  if (is == ok) return;
  if (ok) atomicOr(w, b); else atomicAnd(w, ~b);
}

// target[wrap(map[i])] = src[i] (scalar: src[0]).  BITS: the validity bit of every written row follows in the same pass -- right
// when every candidate of a row carries the same validity (a scalar, or a source without nulls).
template <typename T, bool BITS>
__global__ void __launch_bounds__(COPY_BT) k_scatter(ValueSrc from, const int32_t* __restrict__ map, int64_t n, T* __restrict__ target,
                                                     uint32_t* __restrict__ target_valid, int64_t target_rows)
{
  const T* __restrict__ src = static_cast<const T*>(from.data);
  const int64_t stride      = (int64_t)gridDim.x * COPY_BT;
  const bool ok             = from.scalar_ok();
  for (int64_t i = (int64_t)blockIdx.x * COPY_BT + threadIdx.x; i < n; i += stride) {
    const int64_t m = wrap_row(map[i], target_rows);
    target[m]       = from.is_scalar ? src[0] : src[i];
    if (BITS) put_bit(target_valid, m, ok);
  }
}

// The validity bits of a scatter whose source has nulls, as a pass BEHIND the values: row i writes its bit only where the target
// holds its value.  A map that repeats a target row leaves one candidate's value there; every row that writes the bit carries
// that value, so value and validity of the row come from one candidate.
template <typename T>
__global__ void __launch_bounds__(COPY_BT) k_scatter_bits(const T* __restrict__ src, const uint32_t* __restrict__ src_valid,
                                                          int64_t src_begin_bit, const int32_t* __restrict__ map, int64_t n,
                                                          const T* __restrict__ target, uint32_t* __restrict__ target_valid,
                                                          int64_t target_rows)
{
  const int64_t stride = (int64_t)gridDim.x * COPY_BT;
  for (int64_t i = (int64_t)blockIdx.x * COPY_BT + threadIdx.x; i < n; i += stride) {
    const int64_t m = wrap_row(map[i], target_rows);
    if (target[m] == src[i]) put_bit(target_valid, m, bit_is_set(src_valid, src_begin_bit + i));
  }
}

static inline unsigned copy_grid(int64_t n) { return capped_grid(n, COPY_BT * 4, 8192); }

template <typename T>
int scatter_launch(const void* src, const uint32_t* src_valid, int64_t src_begin_bit, const uint8_t* scalar_valid, int is_scalar,
                   const int32_t* map, int64_t n, void* target, uint32_t* target_valid, int64_t target_rows, hipStream_t s)
{
  const dim3 grid(copy_grid(n)), block(COPY_BT);
  const bool two_passes = target_valid && src_valid && !is_scalar;
  const ValueSrc from{src, src_valid, src_begin_bit, scalar_valid, is_scalar};
  if (target_valid && !two_passes)
    hipLaunchKernelGGL((k_scatter<T, true>), grid, block, 0, s, from, map, n, static_cast<T*>(target), target_valid, target_rows);
  else
    hipLaunchKernelGGL((k_scatter<T, false>), grid, block, 0, s, from, map, n, static_cast<T*>(target), target_valid, target_rows);
  GX_LAUNCH_CHECK();
  if (two_passes) {
    hipLaunchKernelGGL((k_scatter_bits<T>), grid, block, 0, s, static_cast<const T*>(src), src_valid, src_begin_bit, map, n,
                       static_cast<const T*>(target), target_valid, target_rows);
    GX_LAUNCH_CHECK();
  }
  return 0;
}

// ---------------------------------------------------------------- copy_if_else
// out[i] = pick ? lhs[i] : rhs[i], pick = mask[i] != 0 and the mask's bit set.  One row per lane; a wave covers an aligned span of
// 64 rows, reads its 64 bits of each bitmap once (bits_from64: scalar loads) and writes two validity words.
template <typename T, bool HAS_VALID>
__global__ void __launch_bounds__(COPY_BT) k_copy_if_else(ValueSrc lhs, ValueSrc rhs, const uint8_t* __restrict__ mask,
                                                          const uint32_t* __restrict__ mask_valid, int64_t mask_begin_bit, int64_t n,
                                                          T* __restrict__ out, uint32_t* __restrict__ out_valid,
                                                          unsigned long long* __restrict__ null_count)
{
  __shared__ unsigned long long s_nulls;
  const T* __restrict__ lp = static_cast<const T*>(lhs.data);
  const T* __restrict__ rp = static_cast<const T*>(rhs.data);
  const bool l_ok = lhs.scalar_ok(), r_ok = rhs.scalar_ok();
  if (HAS_VALID && null_count) tally_begin(&s_nulls);
  const int64_t n64    = (n + 63) & ~int64_t(63);
  const int64_t stride = (int64_t)gridDim.x * COPY_BT;
  const unsigned lane  = lane_id();
  unsigned long long nulls = 0;
  for (int64_t i = (int64_t)blockIdx.x * COPY_BT + threadIdx.x; i < n64; i += stride) {
    // first row of this wave's span, made wave-uniform for the scalar bitmap loads
    const int64_t i0  = i - lane;
    const int64_t w0  = ((int64_t)__builtin_amdgcn_readfirstlane((int)(i0 >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)i0);
    const int64_t end = w0 + 64 < n ? w0 + 64 : n;  // rows of the span that exist
    const bool live   = i < n;
    bool pick         = live && mask[i] != 0;
    uint64_t pickbits = ballot(pick);
    if (mask_valid) pickbits &= bits_from64(mask_valid, mask_begin_bit + w0, mask_begin_bit + end);
    pick = (pickbits >> lane) & 1u;
    if (live) {
      const T l = lp[lhs.is_scalar ? 0 : i];
      const T r = rp[rhs.is_scalar ? 0 : i];
      out[i]    = pick ? l : r;
    }
    if (HAS_VALID) {
      // the bits of the span's rows; both are 0 from row `end` on, so the row's own bit decides alone
      const uint64_t lbits = lhs.bits64(w0, end, l_ok), rbits = rhs.bits64(w0, end, r_ok);
      const uint64_t b     = (pickbits & lbits) | (~pickbits & rbits);
      store_wave_words(out_valid, w0, n, b);
      nulls += (unsigned long long)((end - w0) - __builtin_popcountll(b));  // (wave-uniform: lane 0's count is the wave's)
    }
  }
  if (HAS_VALID && null_count) tally_end(&s_nulls, nulls, null_count);
}

template <typename T>
int copy_if_else_launch(const ValueSrc& lhs, const ValueSrc& rhs, const uint8_t* mask, const uint32_t* mask_valid, int64_t mask_begin_bit,
                        int64_t n, void* out, uint32_t* out_valid, int64_t* nulls, hipStream_t s)
{
  const dim3 grid(copy_grid(n)), block(COPY_BT);
  if (out_valid)
    hipLaunchKernelGGL((k_copy_if_else<T, true>), grid, block, 0, s, lhs, rhs, mask, mask_valid, mask_begin_bit, n, static_cast<T*>(out),
                       out_valid, reinterpret_cast<unsigned long long*>(nulls));
  else
    hipLaunchKernelGGL((k_copy_if_else<T, false>), grid, block, 0, s, lhs, rhs, mask, mask_valid, mask_begin_bit, n, static_cast<T*>(out),
                       out_valid, reinterpret_cast<unsigned long long*>(nulls));
  GX_LAUNCH_CHECK();
  return 0;
}

constexpr int64_t MAX_ROWS = (int64_t(1) << 31) - 1;

}  // namespace gx

extern "C" {

int gx_concat_tile_rows(void) { return gx::CONCAT_TILE; }

int gx_concatenate(int elem_size, int ninputs, const void* const* cols_host, const int64_t* rows_host,
                   const uint32_t* const* valid_ptrs_host, const int64_t* begin_bits_host, void* out, uint32_t* out_valid,
                   int64_t* out_null_count_dev, void* tmp, size_t* tmp_bytes, gx_stream_t s)
{
  if (elem_size != 1 && elem_size != 2 && elem_size != 4 && elem_size != 8) return GX_EDTYPE;
  if (ninputs < 1 || !tmp_bytes) return GX_EINVAL;
  gx::Carver cv(tmp);
  long long* start       = cv.take<long long>((size_t)ninputs + 1);
  const char** src       = cv.take<const char*>((size_t)ninputs);
  const uint32_t** valid = cv.take<const uint32_t*>((size_t)ninputs);
  long long* bbit        = cv.take<long long>((size_t)ninputs);
  if (int rc; !cv.ready(tmp_bytes, &rc)) return rc;
  if ((!cols_host && out) || !rows_host) return GX_EINVAL;
  int64_t n = 0;
  for (int k = 0; k < ninputs; ++k) {
    if (rows_host[k] < 0 || rows_host[k] > gx::MAX_ROWS) return GX_EINVAL;
    n += rows_host[k];
    if (n > gx::MAX_ROWS) return GX_EINVAL;
    if (rows_host[k] > 0 && !cols_host[k] && out) return GX_EINVAL;
    if (begin_bits_host && begin_bits_host[k] < 0) return GX_EINVAL;
  }
  if (n == 0) return 0;
  if (!out && !out_valid) return GX_EINVAL;
  if (out_null_count_dev) GX_HIP_TRY(hipMemsetAsync(out_null_count_dev, 0, sizeof(int64_t), s));
  long long run = 0;
  for (int base = 0; base < ninputs; base += gx::CONCAT_DESC_BATCH) {
    gx::ConcatDescBatch b{};
    b.base  = base;
    b.count = ninputs - base < gx::CONCAT_DESC_BATCH ? ninputs - base : gx::CONCAT_DESC_BATCH;
    for (int j = 0; j < b.count; ++j) {
      const int k = base + j;
      b.start[j]  = run;
      b.src[j]    = cols_host ? static_cast<const char*>(cols_host[k]) : nullptr;
      b.valid[j]  = valid_ptrs_host ? valid_ptrs_host[k] : nullptr;
      b.bbit[j]   = begin_bits_host ? begin_bits_host[k] : 0;
      run += rows_host[k];
    }
    b.last  = base + b.count == ninputs;
    b.total = run;
    hipLaunchKernelGGL(gx::k_concat_put_desc, dim3(1), dim3(gx::CONCAT_DESC_BATCH), 0, s, b, start, src, valid, bbit);
    GX_LAUNCH_CHECK();
  }
  const gx::ConcatDesc d{start, src, valid, bbit, ninputs};
  return gx::with_width(elem_size, [&](auto tag) { return gx::concat_launch<decltype(tag)>(d, n, out, out_valid, out_null_count_dev, s); });
}

int gx_scatter(int elem_size, const void* src, const uint32_t* src_valid, int64_t src_begin_bit, const uint8_t* src_scalar_valid_dev,
               int src_is_scalar, const int32_t* map, int64_t n, void* target, uint32_t* target_valid, int64_t target_rows,
               gx_stream_t s)
{
  if (elem_size != 1 && elem_size != 2 && elem_size != 4 && elem_size != 8) return GX_EDTYPE;
  if (n < 0 || n > gx::MAX_ROWS || target_rows < 0 || target_rows > gx::MAX_ROWS || src_begin_bit < 0) return GX_EINVAL;
  if (n == 0) return 0;
  if (!src || !map || !target || target_rows == 0) return GX_EINVAL;
  if (src_is_scalar) src_valid = nullptr;
  return gx::with_width(elem_size, [&](auto tag) {
    return gx::scatter_launch<decltype(tag)>(src, src_valid, src_begin_bit, src_scalar_valid_dev, src_is_scalar, map, n, target, target_valid,
                                             target_rows, s);
  });
}

int gx_copy_if_else(int elem_size, const void* lhs, const uint32_t* lhs_valid, int64_t lhs_begin_bit, const uint8_t* lhs_scalar_valid_dev,
                    int lhs_is_scalar, const void* rhs, const uint32_t* rhs_valid, int64_t rhs_begin_bit,
                    const uint8_t* rhs_scalar_valid_dev, int rhs_is_scalar, const uint8_t* mask_bool8, const uint32_t* mask_valid,
                    int64_t mask_begin_bit, int64_t n, void* out, uint32_t* out_valid, int64_t* out_null_count_dev, gx_stream_t s)
{
  if (elem_size != 1 && elem_size != 2 && elem_size != 4 && elem_size != 8) return GX_EDTYPE;
  if (n < 0 || n > gx::MAX_ROWS || lhs_begin_bit < 0 || rhs_begin_bit < 0 || mask_begin_bit < 0) return GX_EINVAL;
  if (n == 0) return 0;
  if (!lhs || !rhs || !mask_bool8 || !out) return GX_EINVAL;
  if (out_null_count_dev) GX_HIP_TRY(hipMemsetAsync(out_null_count_dev, 0, sizeof(int64_t), s));
  const gx::ValueSrc l{lhs, lhs_is_scalar ? nullptr : lhs_valid, lhs_begin_bit, lhs_scalar_valid_dev, lhs_is_scalar};
  const gx::ValueSrc r{rhs, rhs_is_scalar ? nullptr : rhs_valid, rhs_begin_bit, rhs_scalar_valid_dev, rhs_is_scalar};
  return gx::with_width(elem_size, [&](auto tag) {
    return gx::copy_if_else_launch<decltype(tag)>(l, r, mask_bool8, mask_valid, mask_begin_bit, n, out, out_valid, out_null_count_dev, s);
  });
}

}  // extern "C"
