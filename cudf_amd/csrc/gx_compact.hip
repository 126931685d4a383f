// gx_compact.hip -- ordered (stable) stream compaction of fixed-width columns: the kernels behind
// cudf::apply_boolean_mask / drop_nulls / drop_nans (include/cudf/stream_compaction.hpp).
// Replaces thrust::copy_if / cudf::detail::copy_if of the reference (src/stream_compaction/apply_boolean_mask.cu,
// drop_nulls.cu, drop_nans.cu; include/cudf/detail/copy_if.cuh).
//
// Three stages, every one a plain launch (no look-back chain: the selection pass moves <= 1 B/row, a chain would save nothing):
//   select   one selection bit per row as uint64 ballot words + the set bits of every 4096-row chunk (the geometry of the semi
//            join's k_contains, gx_join.hip);
//   scan     scan::k_partials_scan over the chunk counts -> chunk starts, the total behind them;
//   scatter  once per column: out[chunk start + popcount(earlier words of the chunk) + popcount(lower lanes)] = in[row].  Columns
//            without a bitmap go through an LDS stage and leave as 16-byte lanes (k_compact_staged: 2.1 ms against 2.8 ms for the
//            direct k_compact per 1e9 int64 rows at half selectivity, 0.53 against 1.96 ms for int8); columns with one take
//            k_compact, which compacts the validity bits the same way.
// The bits and the chunk starts are the PLAN: one plan serves every column of a table.
// Traffic of apply_boolean_mask on one column of `e` bytes at selectivity s: n * (1 + e * (1 + s)) + n / 4 bytes.
#include "gx_compact.hpp"

namespace gx {
namespace compact {

// the plan, the predicate select kernel and the stages behind it: gx_compact.hpp (shared with gx_distinct.hip)
static std::atomic<int> g_scatter{0};  // A/B knob (gx_knobs.h): 0 = default, 1 = the direct scatter, 2 = the LDS-staged one
constexpr bool STAGED_BY_DEFAULT = true;  // measured: profiles/xp_compaction_mi355x.txt (2.1 vs 2.8 ms per 1e9 int64 rows at s = 0.5)

__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t w)
{
  return ((w & 0xFFu) ? 1u : 0u) | ((w & 0xFF00u) ? 2u : 0u) | ((w & 0xFF0000u) ? 4u : 0u) | ((w & 0xFF000000u) ? 8u : 0u);
}

// ---------------------------------------------------------------------------------------------- select
// BOOL8 mask at 16 rows per lane (the mask pointer is 16-byte aligned): wave w of the chunk owns its rows [w, w + 1) * 1024, lane l
// the 16 of them from 16 l on; the four lanes of a quad hold one ballot word between them.
__global__ void __launch_bounds__(256) k_select_mask16(const uint8_t* __restrict__ mask, const uint32_t* __restrict__ valid,
                                                       int64_t vbit0, int64_t n, uint64_t* __restrict__ bits,
                                                       long long* __restrict__ chunk_count)
{
  __shared__ unsigned int s_cnt;
  const unsigned lane = lane_id();
  const unsigned w    = threadIdx.x / GX_WAVE;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * SEL_CHUNK;
  const int64_t r    = base + (int64_t)w * (16 * GX_WAVE) + (int64_t)lane * 16;
  uint32_t m16       = 0;
  if (r + 16 <= n) {
    const uint4 v = *reinterpret_cast<const uint4*>(mask + r);
    m16           = nonzero_bytes(v.x) | (nonzero_bytes(v.y) << 4) | (nonzero_bytes(v.z) << 8) | (nonzero_bytes(v.w) << 12);
  } else if (r < n) {
    for (int j = 0; j < (int)(n - r); ++j) m16 |= (mask[r + j] != 0 ? 1u : 0u) << j;
  }
  if (valid && r < n) m16 &= bits_from(valid, vbit0 + r, (n - r) < 16 ? (int)(n - r) : 16);
  uint64_t x = (uint64_t)m16 << (16 * (lane & 3u));
  x |= shfl_xor(x, 1);
  x |= shfl_xor(x, 2);
  const int64_t row0 = base + (int64_t)w * (16 * GX_WAVE) + (int64_t)(lane >> 2) * GX_WAVE;  // first row of the quad's word
  if ((lane & 3u) == 0 && row0 < n) bits[row0 >> 6] = x;
  const unsigned int c = wave_reduce((unsigned int)__builtin_popcount(m16), SumOp());
  if (lane == 0 && c) atomicAdd(&s_cnt, c);
  __syncthreads();
  if (threadIdx.x == 0) chunk_count[blockIdx.x] = s_cnt;
}

struct MaskPred {  // BOOL8 mask at any alignment
  const uint8_t* mask;
  const uint32_t* valid;
  int64_t vbit0;
  __device__ __forceinline__ bool operator()(int64_t i) const
  {
    return mask[i] != 0 && (!valid || bit_is_set(valid, vbit0 + i));
  }
};
struct ValidCountPred {  // number of valid keys >= thr (the bitmaps alone: keys.col is not set)
  rows::Cols<MAX_KEYS> keys;
  int thr;
  __device__ __forceinline__ bool operator()(int64_t i) const
  {
    int c = 0;
    for (int k = 0; k < keys.n; ++k) c += keys.is_valid(k, i) ? 1 : 0;
    return c >= thr;
  }
};
struct NotNanPred {  // number of keys that are not NaN >= thr (a key that is no float: its validity alone counts)
  rows::Cols<MAX_KEYS> keys;
  int thr, null_is_missing;
  __device__ __forceinline__ bool operator()(int64_t i) const
  {
    int c = 0;
    for (int k = 0; k < keys.n; ++k) {
      const bool ok = keys.is_valid(k, i);
      bool nan      = false;
      if (ok && keys.kind[k] == K_FLOAT) {  // a null element is not a NaN (its bytes are not looked at)
        if (keys.width[k] == 8) nan = rows::is_nan_bits(static_cast<const uint64_t*>(keys.col[k])[i]);
        else nan = rows::is_nan_bits(static_cast<const uint32_t*>(keys.col[k])[i]);
      }
      c += (null_is_missing ? (ok && !nan) : !nan) ? 1 : 0;
    }
    return c >= thr;
  }
};

// ---------------------------------------------------------------------------------------------- scatter
// Validity: per wave-row the selected lanes are ranked; lane r receives the validity bit of the r-th selected lane (one
// ds_permute: selected lanes go to their rank, the others fill the lanes behind them), a ballot makes the compacted piece of
// popcount(word) bits, and lanes 0..2 OR its (up to three) 32-bit parts into the zeroed output bitmap.
template <typename T, bool HAS_VALID>
__global__ void __launch_bounds__(256) k_compact(const T* __restrict__ in, const uint32_t* __restrict__ in_valid, int64_t vbit0,
                                                 int64_t n, const uint64_t* __restrict__ bits,
                                                 const long long* __restrict__ chunk_start, T* __restrict__ out,
                                                 uint32_t* __restrict__ out_valid, unsigned long long* __restrict__ out_nulls)
{
  __shared__ unsigned int s_row[SEL_WORDS];
  __shared__ unsigned int s_nulls;
  const int64_t base   = (int64_t)blockIdx.x * SEL_CHUNK;
  const int64_t nwords = div_up(n, (int64_t)GX_WAVE);
  if (threadIdx.x < GX_WAVE) {  // exclusive popcount scan of the chunk's 64 words
    const int64_t wi     = (base >> 6) + threadIdx.x;
    const unsigned int c = wi < nwords ? (unsigned int)__builtin_popcountll(bits[wi]) : 0u;
    const unsigned int s = wave_inclusive_scan(c, SumOp());
    s_row[threadIdx.x]   = s - c;
  }
  tally_begin(&s_nulls);  // (its barrier publishes s_row as well)
  const unsigned lane   = lane_id();
  const unsigned w      = threadIdx.x / GX_WAVE;
  const long long start = chunk_start[blockIdx.x];
  unsigned int nulls    = 0;
  for (int k = w; k < SEL_WORDS; k += 256 / GX_WAVE) {
    const int64_t wi = (base >> 6) + k;
    if (wi >= nwords) break;
    const uint64_t b = bits[wi];
    if (b == 0) continue;  // (wave-uniform)
    const int64_t i      = base + (int64_t)k * GX_WAVE + lane;
    const bool sel       = (b >> lane) & 1ull;  // set bits are rows < n
    const unsigned r     = (unsigned)__builtin_popcountll(b & lanemask_lt());
    const long long pos0 = start + s_row[k];
    if (sel) out[pos0 + r] = in[i];
    if (HAS_VALID) {
      const unsigned cnt  = (unsigned)__builtin_popcountll(b);
      const int v         = (sel && bit_is_set(in_valid, vbit0 + i)) ? 1 : 0;
      const unsigned dest = sel ? r : cnt + (lane - r);
      const int got       = __builtin_amdgcn_ds_permute((int)(dest << 2), v);
      const uint64_t piece = ballot(got != 0);  // bit j = validity of the j-th selected row of this word; bits >= cnt are 0
      nulls += cnt - (unsigned)__builtin_popcountll(piece);
      const int sh      = (int)(pos0 & 31);
      const uint64_t lo = piece << sh;
      const uint32_t hi = sh ? (uint32_t)(piece >> (64 - sh)) : 0u;
      const uint32_t part = lane == 0 ? (uint32_t)lo : lane == 1 ? (uint32_t)(lo >> 32) : hi;
      if (lane < 3 && part) atomicOr(&out_valid[(pos0 >> 5) + lane], part);  // set bits lie below the output's row count
    }
  }
  if (HAS_VALID) tally_end(&s_nulls, nulls, out_nulls);
}

// The same scatter with the chunk's selected elements STAGED in LDS and written as whole 16-byte lanes (columns without a bitmap,
// 16-byte aligned output): all 16 element loads of a lane are in flight before the first is used, and the chunk's output run
// [start, start + total) leaves as full-wave 16-byte stores whatever the element size -- the stage is shifted by start mod (16 /
// sizeof(T)) elements so that LDS and global addresses share their alignment; only the run's ragged ends are element stores.
template <typename T>
__global__ void __launch_bounds__(256) k_compact_staged(const T* __restrict__ in, int64_t n, const uint64_t* __restrict__ bits,
                                                        const long long* __restrict__ chunk_start, T* __restrict__ out)
{
  constexpr unsigned VEC = 16 / sizeof(T);
  constexpr int ROWS     = SEL_WORDS / (256 / GX_WAVE);  // wave-rows per wave
  __shared__ unsigned int s_row[SEL_WORDS];
  __shared__ uint64_t s_bits[SEL_WORDS];
  __shared__ unsigned int s_total;
  __shared__ __attribute__((aligned(16))) T s_stage[SEL_CHUNK + VEC];
  const int64_t base   = (int64_t)blockIdx.x * SEL_CHUNK;
  const int64_t nwords = div_up(n, (int64_t)GX_WAVE);
  if (threadIdx.x < GX_WAVE) {
    const int64_t wi     = (base >> 6) + threadIdx.x;
    const uint64_t b     = wi < nwords ? bits[wi] : 0ull;
    const unsigned int c = (unsigned int)__builtin_popcountll(b);
    const unsigned int s = wave_inclusive_scan(c, SumOp());
    s_bits[threadIdx.x]  = b;
    s_row[threadIdx.x]   = s - c;
    if (threadIdx.x == GX_WAVE - 1) s_total = s;
  }
  __syncthreads();
  const unsigned total = s_total;
  if (total == 0) return;  // (uniform over the workgroup)
  const unsigned lane   = lane_id();
  const unsigned w      = threadIdx.x / GX_WAVE;
  const long long start = chunk_start[blockIdx.x];
  const unsigned off    = (unsigned)(start & (long long)(VEC - 1));
  T v[ROWS];
#pragma unroll
  for (int j = 0; j < ROWS; ++j) {
    const int k      = (int)w + j * (256 / GX_WAVE);
    const uint64_t b = s_bits[k];
    v[j]             = ((b >> lane) & 1ull) ? in[base + (int64_t)k * GX_WAVE + lane] : T(0);  // set bits are rows < n
  }
#pragma unroll
  for (int j = 0; j < ROWS; ++j) {
    const int k      = (int)w + j * (256 / GX_WAVE);
    const uint64_t b = s_bits[k];
    if ((b >> lane) & 1ull) s_stage[off + s_row[k] + (unsigned)__builtin_popcountll(b & lanemask_lt())] = v[j];
  }
  __syncthreads();
  // stage[off + j] -> out[start + j], j in [0, total): element stores up to the first 16-byte boundary, 16-byte lanes, the tail
  unsigned head = (VEC - off) & (VEC - 1);
  if (head > total) head = total;
  if (threadIdx.x < head) out[start + threadIdx.x] = s_stage[off + threadIdx.x];
  const unsigned nvec = (total - head) / VEC;
  const uint4* sv     = reinterpret_cast<const uint4*>(s_stage + off + head);
  uint4* ov           = reinterpret_cast<uint4*>(out + start + head);
  for (unsigned q = threadIdx.x; q < nvec; q += 256) ov[q] = sv[q];
  const unsigned done = head + nvec * VEC;
  if (threadIdx.x < total - done) out[start + done + threadIdx.x] = s_stage[off + done + threadIdx.x];
}

// the ascending list of selected rows (k_emit_selected of the semi join, fed by any selector)
__global__ void __launch_bounds__(256) k_compact_indices(const uint64_t* __restrict__ bits, int64_t n,
                                                         const long long* __restrict__ chunk_start, int32_t* __restrict__ out)
{
  __shared__ unsigned int s_row[SEL_WORDS];
  const int64_t base   = (int64_t)blockIdx.x * SEL_CHUNK;
  const int64_t nwords = div_up(n, (int64_t)GX_WAVE);
  if (threadIdx.x < GX_WAVE) {
    const int64_t wi     = (base >> 6) + threadIdx.x;
    const unsigned int c = wi < nwords ? (unsigned int)__builtin_popcountll(bits[wi]) : 0u;
    const unsigned int s = wave_inclusive_scan(c, SumOp());
    s_row[threadIdx.x]   = s - c;
  }
  __syncthreads();
  const unsigned lane   = lane_id();
  const unsigned w      = threadIdx.x / GX_WAVE;
  const long long start = chunk_start[blockIdx.x];
  for (int k = w; k < SEL_WORDS; k += 256 / GX_WAVE) {
    const int64_t wi = (base >> 6) + k;
    if (wi >= nwords) break;
    const uint64_t b = bits[wi];
    if ((b >> lane) & 1ull) out[start + s_row[k] + __builtin_popcountll(b & lanemask_lt())] = (int32_t)(base + (int64_t)k * GX_WAVE + lane);
  }
}

template <typename T>
int compact_launch(const void* in, const uint32_t* in_valid, int64_t vbit0, int64_t n, const Plan& p, void* out, uint32_t* out_valid,
                   int64_t* out_nulls, hipStream_t s)
{
  const int kernel = g_scatter.load(std::memory_order_relaxed);
  const bool wide  = kernel == 2 || (kernel == 0 && STAGED_BY_DEFAULT);
  if (!in_valid && wide && (reinterpret_cast<uintptr_t>(out) & 15u) == 0) {
    hipLaunchKernelGGL((k_compact_staged<T>), dim3((unsigned)p.nchunks), dim3(256), 0, s, static_cast<const T*>(in), n, p.bits, p.starts,
                       static_cast<T*>(out));
    GX_LAUNCH_CHECK();
    return 0;
  }
  if (in_valid)
    hipLaunchKernelGGL((k_compact<T, true>), dim3((unsigned)p.nchunks), dim3(256), 0, s, static_cast<const T*>(in), in_valid, vbit0, n,
                       p.bits, p.starts, static_cast<T*>(out), out_valid, reinterpret_cast<unsigned long long*>(out_nulls));
  else
    hipLaunchKernelGGL((k_compact<T, false>), dim3((unsigned)p.nchunks), dim3(256), 0, s, static_cast<const T*>(in), in_valid, vbit0, n,
                       p.bits, p.starts, static_cast<T*>(out), out_valid, reinterpret_cast<unsigned long long*>(out_nulls));
  GX_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------- compare with a scalar
enum { CMP_EQ = 0, CMP_NE, CMP_LT, CMP_LE, CMP_GT, CMP_GE };

template <typename T>
__global__ void __launch_bounds__(256) k_compare_scalar(const T* __restrict__ in, const uint32_t* __restrict__ valid, int64_t n, int cmp,
                                                        T s, uint8_t* __restrict__ out)
{
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const T v = in[i];
    bool r;
    switch (cmp) {
      case CMP_EQ: r = v == s; break;
      case CMP_NE: r = v != s; break;
      case CMP_LT: r = v < s; break;
      case CMP_LE: r = v <= s; break;
      case CMP_GT: r = v > s; break;
      default: r = v >= s; break;
    }
    if (valid && !bit_is_set(valid, i)) r = false;  // a null row: the byte is defined, the shared bitmap says null
    out[i] = r ? 1 : 0;
  }
}

template <typename T>
int compare_launch(const void* in, const uint32_t* valid, int64_t n, int cmp, uint64_t scalar_bits, uint8_t* out, hipStream_t s)
{
  T sc;
  __builtin_memcpy(&sc, &scalar_bits, sizeof(T));  // the low bytes hold the scalar in the column's type
  hipLaunchKernelGGL((k_compare_scalar<T>), dim3(capped_grid(n, 256 * 8, 8192)), dim3(256), 0, s, static_cast<const T*>(in), valid, n, cmp, sc, out);
  GX_LAUNCH_CHECK();
  return 0;
}

// what every selector does around its kernel; returns 1 when the caller has nothing left to do
static inline int select_prologue(int64_t n, void* tmp, size_t* tmp_bytes, int64_t* count_dev, Plan& p, hipStream_t s, int& rc)
{
  p = carve(tmp, n);
  if (!scratch_ready(tmp, p.bytes, tmp_bytes, &rc)) return 1;
  if (n == 0) {
    rc = 0;
    if (count_dev) {
      hipError_t e = hipMemsetAsync(count_dev, 0, sizeof(int64_t), s);
      if (e != hipSuccess) rc = (int)e;
    }
    return 1;
  }
  return 0;
}

}  // namespace compact
}  // namespace gx

extern "C" {

using namespace gx;
using namespace gx::compact;

void gx_select_set_stages(int mask) { g_stages.store(mask & 3, std::memory_order_relaxed); }
void gx_compact_set_kernel(int kernel) { g_scatter.store(kernel >= 0 && kernel <= 2 ? kernel : 0, std::memory_order_relaxed); }

size_t gx_compact_plan_bytes(int64_t n) { return check_rows(n) ? 0 : carve(nullptr, n).bytes; }

int gx_select_mask(const uint8_t* mask, const uint32_t* mask_valid, int64_t mask_valid_begin_bit, int64_t n, int64_t* count_dev,
                   void* sel_tmp, size_t* tmp_bytes, gx_stream_t stream)
{
  if (check_rows(n) || !tmp_bytes || mask_valid_begin_bit < 0) return GX_EINVAL;
  if (sel_tmp && n > 0 && !mask) return GX_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  Plan p;
  int rc = 0;
  if (select_prologue(n, sel_tmp, tmp_bytes, count_dev, p, s, rc)) return rc;
  if ((reinterpret_cast<uintptr_t>(mask) & 15u) == 0)
    return run_stages(
      [&] {
        hipLaunchKernelGGL(k_select_mask16, dim3((unsigned)p.nchunks), dim3(256), 0, s, mask, mask_valid, mask_valid_begin_bit, n, p.bits,
                           p.starts);
      },
      p, count_dev, s);
  return select_launch(MaskPred{mask, mask_valid, mask_valid_begin_bit}, n, p, count_dev, s);
}

int gx_select_valid_count(int nkeys, const uint32_t* const* valid_ptrs_host, const int64_t* begin_bits_host, int64_t n,
                          int keep_threshold, int64_t* count_dev, void* sel_tmp, size_t* tmp_bytes, gx_stream_t stream)
{
  if (check_rows(n) || !tmp_bytes || nkeys < 0 || nkeys > MAX_KEYS || keep_threshold < 0) return GX_EINVAL;
  if (sel_tmp && nkeys > 0 && !valid_ptrs_host) return GX_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  Plan p;
  int rc = 0;
  if (select_prologue(n, sel_tmp, tmp_bytes, count_dev, p, s, rc)) return rc;
  ValidCountPred pred{};
  pred.keys.n = nkeys;
  pred.thr    = keep_threshold;
  for (int k = 0; k < nkeys; ++k) {
    pred.keys.valid[k] = valid_ptrs_host[k];
    pred.keys.bit0[k]  = begin_bits_host ? begin_bits_host[k] : 0;
    if (pred.keys.bit0[k] < 0) return GX_EINVAL;
  }
  return select_launch(pred, n, p, count_dev, s);
}

int gx_select_not_nan(int nkeys, const int* dtypes_host, const void* const* cols_host, const uint32_t* const* valid_ptrs_host,
                      const int64_t* begin_bits_host, int64_t n, int keep_threshold, int null_is_missing, int64_t* count_dev,
                      void* sel_tmp, size_t* tmp_bytes, gx_stream_t stream)
{
  if (check_rows(n) || !tmp_bytes || nkeys < 0 || nkeys > MAX_KEYS || keep_threshold < 0) return GX_EINVAL;
  if (nkeys > 0 && !dtypes_host) return GX_EINVAL;
  NotNanPred pred{};
  for (int k = 0; k < nkeys; ++k) {
    int kind, width;
    if (rows::key_kind_width(dtypes_host[k], &kind, &width)) return GX_EDTYPE;
    if (kind != K_FLOAT && !null_is_missing) return GX_EDTYPE;  // only validity can make such a key missing
    pred.keys.kind[k]  = kind;
    pred.keys.width[k] = width;
  }
  if (sel_tmp && nkeys > 0 && !cols_host) return GX_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  Plan p;
  int rc = 0;
  if (select_prologue(n, sel_tmp, tmp_bytes, count_dev, p, s, rc)) return rc;
  pred.keys.n          = nkeys;
  pred.thr             = keep_threshold;
  pred.null_is_missing = null_is_missing ? 1 : 0;
  for (int k = 0; k < nkeys; ++k) {  // (the data of a key that is no float is not read: it may be missing)
    pred.keys.col[k]   = cols_host[k];
    pred.keys.valid[k] = valid_ptrs_host ? valid_ptrs_host[k] : nullptr;
    pred.keys.bit0[k]  = begin_bits_host ? begin_bits_host[k] : 0;
    if (pred.keys.bit0[k] < 0 || (!pred.keys.col[k] && pred.keys.kind[k] == K_FLOAT)) return GX_EINVAL;
  }
  return select_launch(pred, n, p, count_dev, s);
}

int gx_compact_column(int elem_size, const void* in, const uint32_t* in_valid, int64_t in_valid_begin_bit, int64_t n,
                      const void* sel_tmp, void* out, uint32_t* out_valid, int64_t* out_null_count_dev, gx_stream_t stream)
{
  if (elem_size != 1 && elem_size != 2 && elem_size != 4 && elem_size != 8) return GX_EDTYPE;
  if (check_rows(n) || in_valid_begin_bit < 0) return GX_EINVAL;
  if (n > 0 && (!in || !out || !sel_tmp)) return GX_EINVAL;
  if (in_valid && !out_valid) return GX_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (out_null_count_dev) GX_HIP_TRY(hipMemsetAsync(out_null_count_dev, 0, sizeof(int64_t), s));
  if (n == 0) return 0;
  const Plan p = carve(sel_tmp, n);
  return with_width(elem_size, [&](auto tag) {
    return compact_launch<decltype(tag)>(in, in_valid, in_valid_begin_bit, n, p, out, out_valid, out_null_count_dev, s);
  });
}

int gx_compact_indices(int64_t n, const void* sel_tmp, int32_t* out_idx, gx_stream_t stream)
{
  if (check_rows(n)) return GX_EINVAL;
  if (n > 0 && (!sel_tmp || !out_idx)) return GX_EINVAL;
  if (n == 0) return 0;
  const Plan p = carve(sel_tmp, n);
  hipLaunchKernelGGL(k_compact_indices, dim3((unsigned)p.nchunks), dim3(256), 0, (hipStream_t)stream, p.bits, n, p.starts, out_idx);
  GX_LAUNCH_CHECK();
  return 0;
}

int gx_compare_scalar(int dtype, const void* in, const uint32_t* in_valid, int64_t n, int cmp, uint64_t scalar_bits, uint8_t* out_bool8,
                      gx_stream_t stream)
{
  if (gx_dtype_size(dtype) == 0) return GX_EDTYPE;
  if (check_rows(n) || cmp < CMP_EQ || cmp > CMP_GE) return GX_EINVAL;
  if (n > 0 && (!in || !out_bool8)) return GX_EINVAL;
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  return with_dtype(dtype, [&](auto t) {
    return compare_launch<typename decltype(t)::value_type>(in, in_valid, n, cmp, scalar_bits, out_bool8, s);
  });
}

}  // extern "C"
