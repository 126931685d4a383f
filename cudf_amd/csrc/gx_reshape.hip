// gx_reshape.hip -- the kernels behind <cudf/reshape.hpp>, <cudf/transpose.hpp> and <cudf/filling.hpp>: interleave (an LDS-staged
// transpose: cudf::interleave_columns and the data movement of cudf::transpose), tile, repeat (scalar count: streaming; count
// column: an expansion map for gx_gather), fill and sequence.  reference: cpp/src/reshape/interleave_columns.cu, tile.cu,
// cpp/src/transpose/transpose.cu, cpp/src/filling/fill.cu, repeat.cu, sequence.cu.  All of them are HBM-bound; values move as
// bits, validity bitmaps are Arrow bitmaps read from a begin bit on (gx_validity.hpp), and every output validity word has one
// owner, so nothing is merged with atomics.
#include "gx_common.hpp"

#include <type_traits>

namespace gx {

constexpr int RS_BT       = 256;
constexpr int64_t RS_MAX  = (int64_t(1) << 31) - 1;
constexpr int RS_TILE     = 2048;  // result rows one workgroup owns per trip in tile / repeat: 64 validity words, 8 rows a thread
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));  // 16 bytes as one access (a native vector: the non-temporal builtins take it)

// ---------------------------------------------------------------- interleave
// Tile: rows x cols of the input a workgroup stages.  Up to IL_BAND_COLS columns a tile holds every column of a band of rows
// (a multiple of 32 rows: the band's output run starts 16-byte aligned whenever `out` is); above, 64 x 32.
constexpr int IL_BAND_COLS  = 32;
constexpr int IL_BAND_BYTES = 16384;
constexpr int IL_BAND_ROWS_MAX = 4096;
constexpr int IL_2D_ROWS    = 64;
constexpr int IL_2D_COLS    = 32;
constexpr int IL_DESC_BATCH = 64;

static inline void interleave_tile(int elem_size, int ncols, int* rows, int* cols)
{
  if (ncols <= IL_BAND_COLS) {
    int r = IL_BAND_BYTES / (ncols * elem_size) / 32 * 32;
    r     = r < 32 ? 32 : (r > IL_BAND_ROWS_MAX ? IL_BAND_ROWS_MAX : r);
    *rows = r;
    *cols = ncols;
  } else {
    *rows = IL_2D_ROWS;
    *cols = IL_2D_COLS;
  }
}

// The LDS image of a tile is its elements in output order (row-major, the tile's columns side by side), with one pad word behind
// every 32 words and one more behind every 1024.  A column's stretch is written into it at a stride of `cols` elements (16-byte
// loads: 16 / sizeof(T) rows a lane, so 4 * cols words between lanes).  ds_write banks are (address / 4) mod 32, counted over 32
// lanes: without padding a power-of-two stride s puts the 32 lanes on 32 / s banks (s = 16: 16-way); with it lane l lands on
// s * l + (s * l >> 5) + (s * l >> 10), which is a different bank for each of the 32 lanes for every power of two s up to 1024.
// A 16-byte chunk of the image (4 words at a multiple of 4) never contains a pad, so the way out reads whole chunks.
__host__ __device__ __forceinline__ uint32_t il_phys(uint32_t byte) { return byte + ((byte >> 7) << 2) + ((byte >> 12) << 2); }
static inline size_t il_lds_bytes(int rows, int cols, int elem_size) { return il_phys((uint32_t)(rows * cols * elem_size)) + 16; }

struct InterleaveDesc {
  const char* const* src;
  const uint32_t* const* valid;  // NULL entry = no nulls
  const long long* bbit;
};
struct InterleaveDescBatch {
  const char* src[IL_DESC_BATCH];
  const uint32_t* valid[IL_DESC_BATCH];
  long long bbit[IL_DESC_BATCH];
  int base, count;
};
__global__ void __launch_bounds__(IL_DESC_BATCH) k_interleave_put_desc(InterleaveDescBatch b, const char** src, const uint32_t** valid,
                                                                       long long* bbit)
{
  const int j = threadIdx.x;
  if (j < b.count) {
    src[b.base + j]   = b.src[j];
    valid[b.base + j] = b.valid[j];
    bbit[b.base + j]  = b.bbit[j];
  }
}

template <typename T>
__device__ __forceinline__ void il_put(char* lds, uint32_t elem, T v)
{
  char* p = lds + il_phys(elem * (uint32_t)sizeof(T));
  if constexpr (sizeof(T) == 8) {  // the image is word aligned only
    reinterpret_cast<uint32_t*>(p)[0] = (uint32_t)v;
    reinterpret_cast<uint32_t*>(p)[1] = (uint32_t)(v >> 32);
  } else {
    *reinterpret_cast<T*>(p) = v;
  }
}
template <typename T>
__device__ __forceinline__ T il_get(const char* lds, uint32_t elem)
{
  const char* p = lds + il_phys(elem * (uint32_t)sizeof(T));
  if constexpr (sizeof(T) == 8) {
    return (T)reinterpret_cast<const uint32_t*>(p)[0] | ((T)reinterpret_cast<const uint32_t*>(p)[1] << 32);
  } else {
    return *reinterpret_cast<const T*>(p);
  }
}

// tile_rows x tile_cols as interleave_tile gives them; tile_cols == ncols: the band regime (one column tile)
template <typename T>
__global__ void __launch_bounds__(RS_BT) k_interleave(InterleaveDesc d, int ncols, int64_t nrows, int tile_rows, int tile_cols,
                                                      int col_tiles, T* __restrict__ out)
{
  extern __shared__ __attribute__((aligned(16))) char il_lds[];
  constexpr int K   = 16 / (int)sizeof(T);  // rows of a 16-byte load
  const unsigned t  = threadIdx.x;
  const int64_t rt  = (int64_t)blockIdx.x / col_tiles;
  const int ct      = (int)((int64_t)blockIdx.x % col_tiles);
  const int64_t r0  = rt * tile_rows;
  const int c0      = ct * tile_cols;
  const int rw      = (int)(nrows - r0 < tile_rows ? nrows - r0 : tile_rows);
  const int cw      = ncols - c0 < tile_cols ? ncols - c0 : tile_cols;

  // in.  Whole 16-byte loads when every column of the tile starts on a 16-byte boundary and the tile's rows divide into them (every
  // tile but a ragged last one, of columns the caller did not misalign): the (column, chunk) pairs are spread over the workgroup,
  // consecutive lanes on consecutive chunks of one column.  Else element by element, the (column, row) pairs spread the same way.
  bool vec = rw % K == 0;
  for (int j = 0; j < cw && vec; ++j) vec = ((reinterpret_cast<uintptr_t>(d.src[c0 + j]) + (uintptr_t)r0 * sizeof(T)) & 15u) == 0;
  if (vec) {
    const uint32_t nv = (uint32_t)rw / K, items = nv * (uint32_t)cw;
#pragma unroll 2
    for (uint32_t it = t; it < items; it += RS_BT) {
      const uint32_t j = it / nv, q = it - j * nv;
      const u32x4 v    = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(reinterpret_cast<const T*>(d.src[c0 + j]) + r0) + q);
      T e[K];
      __builtin_memcpy(e, &v, 16);
#pragma unroll
      for (int k = 0; k < K; ++k) il_put<T>(il_lds, (q * K + k) * (uint32_t)cw + j, e[k]);
    }
  } else {
    const uint32_t items = (uint32_t)rw * (uint32_t)cw;
    for (uint32_t it = t; it < items; it += RS_BT) {
      const uint32_t j = it / (uint32_t)rw, i = it - j * (uint32_t)rw;
      il_put<T>(il_lds, i * (uint32_t)cw + j, (reinterpret_cast<const T*>(d.src[c0 + j]) + r0)[i]);
    }
  }
  __syncthreads();

  // out
  if (cw == ncols) {  // the band: one contiguous run of rw * ncols elements
    T* __restrict__ run  = out + r0 * ncols;
    const uint32_t elems = (uint32_t)rw * (uint32_t)ncols;
    uint32_t done        = 0;
    if ((reinterpret_cast<uintptr_t>(run) & 15u) == 0) {
      const uint32_t nv = elems / K;
      u32x4* __restrict__ rv = reinterpret_cast<u32x4*>(run);
      for (uint32_t q = t; q < nv; q += RS_BT) {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(il_lds + il_phys(q * 16u));
        const u32x4 v     = {w[0], w[1], w[2], w[3]};
        __builtin_nontemporal_store(v, rv + q);
      }
      done = nv * K;
    }
    for (uint32_t i = done + t; i < elems; i += RS_BT) run[i] = il_get<T>(il_lds, i);
  } else {  // two-dimensional: row i of the tile is a run of cw elements at out[(r0 + i) * ncols + c0]
    const uint32_t elems = (uint32_t)rw * (uint32_t)cw;
    for (uint32_t e = t; e < elems; e += RS_BT) {
      const uint32_t i = e / (uint32_t)cw, j = e - i * (uint32_t)cw;
      out[(r0 + i) * ncols + c0 + j] = il_get<T>(il_lds, e);
    }
  }
}

// validity of the interleave: thread = output word.  Output bit i * ncols + j is bit begin_bit_j + i of column j.
__global__ void __launch_bounds__(RS_BT) k_interleave_valid(InterleaveDesc d, int ncols, int64_t total, uint32_t* __restrict__ out_valid,
                                                            unsigned long long* __restrict__ null_count)
{
  __shared__ unsigned int s_nulls;
  tally_begin(&s_nulls);
  const int64_t nwords = (total + 31) >> 5;
  const int64_t w      = (int64_t)blockIdx.x * RS_BT + threadIdx.x;
  unsigned int nulls   = 0;
  if (w < nwords) {
    const int64_t e0 = w * 32;
    const int64_t e1 = e0 + 32 < total ? e0 + 32 : total;
    uint32_t word    = 0;
    if (ncols <= 32) {
      // the word covers rows i0 .. i1 (at most 32 of them): each column's bits for those rows are fetched once
      const int64_t i0 = e0 / ncols, i1 = (e1 - 1) / ncols;
      const int nr     = (int)(i1 - i0 + 1);
      for (int j = 0; j < ncols; ++j) {
        const uint32_t* m   = d.valid[j];
        const uint32_t bits = m ? bits_from(m, d.bbit[j] + i0, nr) : low_mask32(nr);
        for (int ii = 0; ii < nr; ++ii) {
          const int64_t e = (i0 + ii) * ncols + j;
          if (e >= e0 && e < e1) word |= ((bits >> ii) & 1u) << (int)(e - e0);
        }
      }
    } else {
      int64_t i = e0 / ncols;
      int j     = (int)(e0 - i * ncols);
      for (int64_t e = e0; e < e1; ++e) {
        const uint32_t* m = d.valid[j];
        if (!m || bit_is_set(m, d.bbit[j] + i)) word |= 1u << (int)(e - e0);
        if (++j == ncols) {
          j = 0;
          ++i;
        }
      }
    }
    out_valid[w] = word;
    nulls        = (unsigned int)((e1 - e0) - __builtin_popcount(word));
  }
  nulls = wave_reduce(nulls, SumOp());
  tally_end(&s_nulls, nulls, null_count);
}

// ---------------------------------------------------------------- tile / repeat with a scalar count
// MODE 0 (tile): result row e reads in[e mod nrows]; MODE 1 (repeat_each): in[e / count].  A thread walks its rows of the tile at a
// stride of RS_BT and carries the source position along (one division per thread and trip, none per row).
struct WrapPos {
  uint32_t q, r;  // MODE 0: r = e mod nrows (q unused); MODE 1: q = e / count, r = e mod count
};

template <typename T, int MODE>
__global__ void __launch_bounds__(RS_BT) k_tile_repeat(const T* __restrict__ in, const uint32_t* __restrict__ in_valid, int64_t in_begin_bit,
                                                       uint32_t nrows, uint32_t count, int64_t total, T* __restrict__ out,
                                                       uint32_t* __restrict__ out_valid, unsigned long long* __restrict__ null_count)
{
  __shared__ unsigned int s_nulls;
  const unsigned t      = threadIdx.x;
  const uint32_t period = MODE == 0 ? nrows : count;
  const uint32_t step_q = RS_BT / period, step_r = RS_BT % period;
  const int64_t tiles   = div_up(total, RS_TILE);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t t0 = tile * RS_TILE;
    const int64_t t1 = t0 + RS_TILE < total ? t0 + RS_TILE : total;

    // validity: thread j (the first wave) composes word j of the tile
    if (out_valid) {
      if (null_count) tally_begin(&s_nulls);
      unsigned int nulls = 0;
      if (t < RS_TILE / 32) {
        const int64_t e0 = t0 + (int64_t)t * 32;
        if (e0 < t1) {
          const int64_t e1 = e0 + 32 < t1 ? e0 + 32 : t1;
          uint32_t word    = 0;
          if (!in_valid) {
            word = low_mask32((int)(e1 - e0));
          } else if (MODE == 0) {
            // runs of the input bitmap, wrapping at nrows: several inside the word when nrows < 32
            int64_t e = e0;
            int64_t i = e0 % nrows;
            while (e < e1) {
              const int64_t left = (int64_t)nrows - i;
              const int cnt      = (int)(left < e1 - e ? left : e1 - e);
              word |= bits_from(in_valid, in_begin_bit + i, cnt) << (int)(e - e0);
              e += cnt;
              i = 0;
            }
          } else {
            // the word covers source rows i0 .. (e1 - 1) / count, at most 32: their bits are fetched once, each one spread
            // over the result rows of its source row
            const int64_t i0    = e0 / count;
            const int nr        = (int)((e1 - 1) / count - i0 + 1);
            const uint32_t bits = bits_from(in_valid, in_begin_bit + i0, nr);
            for (int ii = 0; ii < nr; ++ii) {
              const int64_t a = (i0 + ii) * count, b = a + count;
              const int64_t lo = a > e0 ? a : e0, hi = b < e1 ? b : e1;
              if ((bits >> ii) & 1u) word |= low_mask32((int)(hi - lo)) << (int)(lo - e0);
            }
          }
          out_valid[e0 >> 5] = word;
          nulls              = (unsigned int)((e1 - e0) - __builtin_popcount(word));
        }
        if (null_count) nulls = wave_reduce(nulls, SumOp());
      }
      if (null_count) tally_end(&s_nulls, nulls, null_count);
    }

    // data
    const int64_t e_first = t0 + t;
    WrapPos p;
    p.q = (uint32_t)(e_first / period);
    p.r = (uint32_t)(e_first % period);
#pragma unroll 4
    for (int64_t e = e_first; e < t1; e += RS_BT) {
      out[e] = in[MODE == 0 ? p.r : p.q];
      p.q += step_q;
      p.r += step_r;
      if (p.r >= period) {
        p.r -= period;
        ++p.q;
      }
    }
  }
}

template <typename T, int MODE>
int tile_repeat_launch(const void* in, const uint32_t* in_valid, int64_t in_begin_bit, int64_t nrows, int64_t count, void* out,
                       uint32_t* out_valid, int64_t* nulls, hipStream_t s)
{
  const int64_t total = nrows * count;
  hipLaunchKernelGGL((k_tile_repeat<T, MODE>), dim3(capped_grid(total, RS_TILE, 16384)), dim3(RS_BT), 0, s, static_cast<const T*>(in), in_valid,
                     in_begin_bit, (uint32_t)nrows, (uint32_t)count, total, static_cast<T*>(out), out_valid,
                     reinterpret_cast<unsigned long long*>(nulls));
  GX_LAUNCH_CHECK();
  return 0;
}

static int tile_repeat(int mode, int elem_size, const void* in, const uint32_t* in_valid, int64_t in_begin_bit, int64_t nrows, int64_t count,
                       void* out, uint32_t* out_valid, int64_t* out_null_count_dev, hipStream_t s)
{
  if (elem_size != 1 && elem_size != 2 && elem_size != 4 && elem_size != 8) return GX_EDTYPE;
  if (nrows < 0 || nrows > RS_MAX || count < 0 || count > RS_MAX || in_begin_bit < 0) return GX_EINVAL;
  if (nrows > 0 && count > RS_MAX / nrows) return GX_EINVAL;
  if (nrows * count == 0) return 0;
  if (!in || !out) return GX_EINVAL;
  if (out_null_count_dev) GX_HIP_TRY(hipMemsetAsync(out_null_count_dev, 0, sizeof(int64_t), s));
  return with_width(elem_size, [&](auto tag) {
    using T = decltype(tag);
    return mode == 0 ? tile_repeat_launch<T, 0>(in, in_valid, in_begin_bit, nrows, count, out, out_valid, out_null_count_dev, s)
                     : tile_repeat_launch<T, 1>(in, in_valid, in_begin_bit, nrows, count, out, out_valid, out_null_count_dev, s);
  });
}

// ---------------------------------------------------------------- repeat with a count column: the expansion map
// offsets[s] = first result row of source row s (nrows + 1 entries, non-decreasing, offsets[nrows] = total).  The source row of
// result row e is the LAST s with offsets[s] <= e: rows of count 0 share their position with the next row that has a count.
__device__ __forceinline__ int repeat_find(const int32_t* __restrict__ offsets, int nrows, int64_t e)
{
  int lo = 0, hi = nrows;  // offsets[0] = 0 <= e; the answer lies in [lo, hi)
  while (hi - lo > 1) {
    const int mid = (int)(((int64_t)lo + hi) >> 1);
    if (offsets[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(RS_BT) k_repeat_map(const int32_t* __restrict__ offsets, int nrows, int64_t total, int32_t* __restrict__ out_map)
{
  constexpr int PER = RS_TILE / RS_BT;  // 8 consecutive result rows a thread
  __shared__ __attribute__((aligned(16))) int32_t marks[RS_TILE];
  __shared__ int32_t scan_lds[RS_BT / GX_WAVE + 1];
  const unsigned t = threadIdx.x;
  const int64_t t0 = (int64_t)blockIdx.x * RS_TILE;
  const int64_t t1 = t0 + RS_TILE < total ? t0 + RS_TILE : total;
  // one binary search for each end of the tile, the same in every lane (scalar loads); a source row that spans many tiles costs
  // each of them these two searches and nothing else
  const int s0 = repeat_find(offsets, nrows, t0);
  const int s1 = repeat_find(offsets, nrows, t1 - 1);
#pragma unroll
  for (int k = 0; k < PER; ++k) marks[t + k * RS_BT] = 0;
  __syncthreads();
  if (t == 0) marks[0] = s0;
  // source rows behind s0 that begin inside the tile.  A row of count 0 begins where the next row begins and loses to it (the
  // largest row number wins): it is skipped, so every position is written by one row and no atomic is needed.  The rows of a run of
  // zero counts are read once, by the tile that holds their position.
  for (int s = s0 + 1 + (int)t; s <= s1; s += RS_BT) {
    const int32_t p = offsets[s];
    if (offsets[s + 1] != p && (uint64_t)(p - t0) < (uint64_t)RS_TILE) marks[p - t0] = s;  // (the range holds for sorted offsets)
  }
  __syncthreads();
  // marks -> row numbers: inclusive running max, 8 consecutive positions a thread, the carries across threads in one block scan
  int32_t v[PER];
  {
    const int4 a = reinterpret_cast<const int4*>(marks)[2 * t], b = reinterpret_cast<const int4*>(marks)[2 * t + 1];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
#pragma unroll
  for (int k = 1; k < PER; ++k) v[k] = v[k] > v[k - 1] ? v[k] : v[k - 1];
  const int32_t carry = block_exclusive_scan<RS_BT>(v[PER - 1], (int32_t)0, MaxOp(), scan_lds, (int32_t*)nullptr);
#pragma unroll
  for (int k = 0; k < PER; ++k) v[k] = v[k] > carry ? v[k] : carry;
  reinterpret_cast<int4*>(marks)[2 * t]     = make_int4(v[0], v[1], v[2], v[3]);
  reinterpret_cast<int4*>(marks)[2 * t + 1] = make_int4(v[4], v[5], v[6], v[7]);
  __syncthreads();
  // out: consecutive lanes, consecutive 16 bytes
  int32_t* __restrict__ run = out_map + t0;
  const uint32_t elems      = (uint32_t)(t1 - t0);
  uint32_t done             = 0;
  if ((reinterpret_cast<uintptr_t>(run) & 15u) == 0) {
    const uint32_t nv = elems / 4;
    for (uint32_t q = t; q < nv; q += RS_BT) reinterpret_cast<int4*>(run)[q] = reinterpret_cast<const int4*>(marks)[q];
    done = nv * 4;
  }
  for (uint32_t i = done + t; i < elems; i += RS_BT) run[i] = marks[i];
}

// ---------------------------------------------------------------- fill
// data[begin, end) = *value: elements up to the first 16-byte boundary, 16-byte stores, elements behind the last
template <typename T>
__global__ void __launch_bounds__(RS_BT) k_fill_range(T* __restrict__ data, int64_t begin, int64_t end, const T* __restrict__ value)
{
  constexpr int K = 16 / (int)sizeof(T);
  const T v       = *value;
  T* p            = data + begin;
  const int64_t n = end - begin;
  int64_t head    = (int64_t)(((0 - reinterpret_cast<uintptr_t>(p)) & 15u) / sizeof(T));  // (p is aligned to its element)
  if (head > n) head = n;
  const int64_t nv     = (n - head) / K;
  const int64_t gid    = (int64_t)blockIdx.x * RS_BT + threadIdx.x;
  if (gid < head) p[gid] = v;
  T e[K];
#pragma unroll
  for (int k = 0; k < K; ++k) e[k] = v;
  uint4 v4;
  __builtin_memcpy(&v4, e, 16);
  uint4* pv = reinterpret_cast<uint4*>(p + head);
  // a workgroup writes 4 x RS_BT consecutive chunks a trip (16 KiB), four stores a thread in flight
  constexpr int64_t TRIP = 4 * RS_BT;
  for (int64_t base = (int64_t)blockIdx.x * TRIP; base < nv; base += (int64_t)gridDim.x * TRIP) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t q = base + u * RS_BT + threadIdx.x;
      if (q < nv) pv[q] = v4;
    }
  }
  const int64_t tail0 = head + nv * K;
  if (gid < n - tail0) p[tail0 + gid] = v;
}

// ---------------------------------------------------------------- sequence
// Integers in the unsigned type of the width (wrap modulo 2^w).  Floats: T(i) * step rounded to T, then init + that rounded to T --
// the two roundings of NumPy's init + arange(n).astype(T) * step.  hipcc contracts a + b * c into one fma (one rounding, another
// last bit) by default: `#pragma clang fp contract(off)` on this function keeps the two operations apart.
template <typename T>
__device__ __forceinline__ T sequence_value(T init, T step, int64_t i)
{
#pragma clang fp contract(off)
  if constexpr (std::is_floating_point<T>::value) {
    const T prod = (T)i * step;
    return init + prod;
  } else {
    return (T)(init + (T)(uint64_t)i * step);
  }
}

template <typename T>
__global__ void __launch_bounds__(RS_BT) k_sequence(T* __restrict__ out, int64_t n, const T* __restrict__ init_p, const T* __restrict__ step_p)
{
  const T init         = *init_p;
  const T step         = step_p ? *step_p : T(1);
  const int64_t stride = (int64_t)gridDim.x * RS_BT;
  for (int64_t i = (int64_t)blockIdx.x * RS_BT + threadIdx.x; i < n; i += stride) out[i] = sequence_value<T>(init, step, i);
}

template <typename T>
int sequence_launch(void* out, int64_t n, const void* init, const void* step, hipStream_t s)
{
  hipLaunchKernelGGL((k_sequence<T>), dim3(capped_grid(n, RS_BT * 4, 8192)), dim3(RS_BT), 0, s, static_cast<T*>(out), n,
                     static_cast<const T*>(init), static_cast<const T*>(step));
  GX_LAUNCH_CHECK();
  return 0;
}

}  // namespace gx

extern "C" {

int gx_reshape_tile_rows(void) { return gx::RS_TILE; }

int gx_interleave_tile(int elem_size, int ncols, int* rows, int* cols)
{
  if (elem_size != 1 && elem_size != 2 && elem_size != 4 && elem_size != 8) return GX_EDTYPE;
  if (ncols < 1 || !rows || !cols) return GX_EINVAL;
  gx::interleave_tile(elem_size, ncols, rows, cols);
  return 0;
}

int gx_interleave(int elem_size, int ncols, const void* const* cols_host, const uint32_t* const* valid_ptrs_host,
                  const int64_t* begin_bits_host, int64_t nrows, void* out, uint32_t* out_valid, int64_t* out_null_count_dev, void* tmp,
                  size_t* tmp_bytes, gx_stream_t s)
{
  if (elem_size != 1 && elem_size != 2 && elem_size != 4 && elem_size != 8) return GX_EDTYPE;
  if (ncols < 1 || !tmp_bytes) return GX_EINVAL;
  gx::Carver cv(tmp);
  const char** src       = cv.take<const char*>((size_t)ncols);
  const uint32_t** valid = cv.take<const uint32_t*>((size_t)ncols);
  long long* bbit        = cv.take<long long>((size_t)ncols);
  if (int rc; !cv.ready(tmp_bytes, &rc)) return rc;
  if (nrows < 0 || nrows > gx::RS_MAX || nrows > gx::RS_MAX / ncols || !cols_host) return GX_EINVAL;
  for (int j = 0; j < ncols; ++j) {
    if (nrows > 0 && !cols_host[j]) return GX_EINVAL;
    if (begin_bits_host && begin_bits_host[j] < 0) return GX_EINVAL;
  }
  if (nrows == 0) return 0;
  if (!out) return GX_EINVAL;
  const int64_t total = nrows * ncols;
  gx::Device dev;
  GX_HIP_TRY(gx::device(&dev));
  if (out_null_count_dev) GX_HIP_TRY(hipMemsetAsync(out_null_count_dev, 0, sizeof(int64_t), s));
  for (int base = 0; base < ncols; base += gx::IL_DESC_BATCH) {
    gx::InterleaveDescBatch b{};
    b.base  = base;
    b.count = ncols - base < gx::IL_DESC_BATCH ? ncols - base : gx::IL_DESC_BATCH;
    for (int j = 0; j < b.count; ++j) {
      b.src[j]   = static_cast<const char*>(cols_host[base + j]);
      b.valid[j] = valid_ptrs_host ? valid_ptrs_host[base + j] : nullptr;
      b.bbit[j]  = begin_bits_host ? begin_bits_host[base + j] : 0;
    }
    hipLaunchKernelGGL(gx::k_interleave_put_desc, dim3(1), dim3(gx::IL_DESC_BATCH), 0, s, b, src, valid, bbit);
    GX_LAUNCH_CHECK();
  }
  const gx::InterleaveDesc d{src, valid, bbit};
  int tr = 0, tc = 0;
  gx::interleave_tile(elem_size, ncols, &tr, &tc);
  const int64_t row_tiles = gx::div_up(nrows, tr);
  const int col_tiles     = (int)gx::div_up(ncols, tc);
  const size_t lds        = gx::il_lds_bytes(tr, tc, elem_size);
  const int rc            = ncols == 1 ? gx_copy_bytes(cols_host[0], out, (size_t)nrows * elem_size, s) : gx::with_width(elem_size, [&](auto tag) {
    using T = decltype(tag);
    GX_HIP_TRY(gx::launch_lds(dev, gx::k_interleave<T>, dim3((unsigned)(row_tiles * col_tiles)), dim3(gx::RS_BT), lds, s, d, ncols, nrows, tr, tc,
                              col_tiles, static_cast<T*>(out)));
    GX_LAUNCH_CHECK();
    return 0;
  });
  if (rc) return rc;
  if (out_valid) {
    const int64_t nwords = (total + 31) / 32;
    hipLaunchKernelGGL(gx::k_interleave_valid, dim3((unsigned)gx::div_up(nwords, gx::RS_BT)), dim3(gx::RS_BT), 0, s, d, ncols, total, out_valid,
                       reinterpret_cast<unsigned long long*>(out_null_count_dev));
    GX_LAUNCH_CHECK();
  }
  return 0;
}

int gx_tile(int elem_size, const void* in, const uint32_t* in_valid, int64_t in_begin_bit, int64_t nrows, int64_t count, void* out,
            uint32_t* out_valid, int64_t* out_null_count_dev, gx_stream_t s)
{
  return gx::tile_repeat(0, elem_size, in, in_valid, in_begin_bit, nrows, count, out, out_valid, out_null_count_dev, s);
}

int gx_repeat_each(int elem_size, const void* in, const uint32_t* in_valid, int64_t in_begin_bit, int64_t nrows, int64_t count, void* out,
                   uint32_t* out_valid, int64_t* out_null_count_dev, gx_stream_t s)
{
  return gx::tile_repeat(1, elem_size, in, in_valid, in_begin_bit, nrows, count, out, out_valid, out_null_count_dev, s);
}

int gx_repeat_map(const int32_t* offsets_dev, int64_t nrows, int64_t total, int32_t* out_map, void* tmp, size_t* tmp_bytes, gx_stream_t s)
{
  if (!tmp_bytes) return GX_EINVAL;
  if (int rc; !gx::scratch_ready(tmp, 0, tmp_bytes, &rc)) return rc;  // no scratch: the query answers 0
  if (nrows < 0 || nrows > gx::RS_MAX || total < 0 || total > gx::RS_MAX || (total > 0 && nrows == 0)) return GX_EINVAL;
  if (total == 0) return 0;
  if (!offsets_dev || !out_map) return GX_EINVAL;
  hipLaunchKernelGGL(gx::k_repeat_map, dim3((unsigned)gx::div_up(total, gx::RS_TILE)), dim3(gx::RS_BT), 0, s, offsets_dev, (int)nrows, total,
                     out_map);
  GX_LAUNCH_CHECK();
  return 0;
}

int gx_fill_range(int elem_size, void* data, int64_t begin, int64_t end, const void* value_dev, gx_stream_t s)
{
  if (elem_size != 1 && elem_size != 2 && elem_size != 4 && elem_size != 8) return GX_EDTYPE;
  if (begin < 0 || end < begin || end > gx::RS_MAX) return GX_EINVAL;
  if (begin == end) return 0;
  if (!data || !value_dev) return GX_EINVAL;
  const int64_t chunks = gx::div_up((end - begin) * elem_size, 16) + 1;
  return gx::with_width(elem_size, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((gx::k_fill_range<T>), dim3(gx::capped_grid(chunks, gx::RS_BT * 4, 16384)), dim3(gx::RS_BT), 0, s, static_cast<T*>(data),
                       begin, end, static_cast<const T*>(value_dev));
    GX_LAUNCH_CHECK();
    return 0;
  });
}

int gx_sequence(int dtype, void* out, int64_t n, const void* init_dev, const void* step_dev, gx_stream_t s)
{
  if (dtype < GX_INT8 || dtype > GX_FLOAT64) return GX_EDTYPE;  // GX_BOOL8 and anything unknown
  if (n < 0 || n > gx::RS_MAX) return GX_EINVAL;
  if (n == 0) return 0;
  if (!out || !init_dev) return GX_EINVAL;
  return gx::with_dtype(dtype, [&](auto t) {  // integers wrap: one kernel per width, the unsigned one
    return gx::sequence_launch<gx::word_or_float_t<decltype(t)>>(out, n, init_dev, step_dev, s);
  });
}

}  // extern "C"
