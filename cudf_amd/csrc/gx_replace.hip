// gx_replace.hip -- the kernels behind <cudf/replace.hpp>: replace_nulls (column, scalar, PRECEDING / FOLLOWING), replace_nans,
// clamp, find_and_replace_all and normalize_nans_and_zeros.  reference: cpp/src/replace (nulls.cu, nans.cu, clamp.cu, replace.cu),
// cpp/include/cudf/replace.hpp.  All of them are streaming passes over Arrow buffers: values move as bits wherever no comparison
// is needed, bitmaps are read from their own begin bit, and a workgroup owns whole validity words (gx_validity.hpp), so no word is
// merged with atomics.  Only the policy fill has scratch (one int32 per tile) and no kernel here waits for another workgroup.
#include "gx_common.hpp"

#include <type_traits>

namespace gx {
namespace rp {

constexpr int BT          = 256;
constexpr int ROWS        = 16;         // rows of one thread per tile: 16 / R accesses of R rows, R = 16 / sizeof(T)
constexpr int TILE        = BT * ROWS;  // rows a workgroup owns per trip: a multiple of 64, so it owns whole validity words
constexpr int WORDS       = TILE / 64;  // 64-row spans of a tile: one per lane of a wave
constexpr int GRID_CAP    = 2048;       // 8 workgroups on each of 256 CUs; further tiles are further trips
constexpr int CARRY_BLOCK = 1024;       // tile-table entries one workgroup of the carry pass scans
constexpr int FR_CHUNK    = 1024;       // old values of find_and_replace staged through LDS at a time
constexpr int64_t MAX_ROWS = (int64_t(1) << 31) - 1;
static_assert(WORDS == GX_WAVE, "the per-word table of a tile is built by one wave, a word per lane");

static inline bool width_ok(int e) { return e == 1 || e == 2 || e == 4 || e == 8; }
static inline bool dtype_ok(int d) { return d >= GX_INT8 && d <= GX_BOOL8; }
static inline bool is_float(int d) { return d == GX_FLOAT32 || d == GX_FLOAT64; }

// R consecutive rows as one 16-byte access where the column's first row is 16-byte aligned (row0 is a multiple of R, so the base
// decides for every access: a wave-uniform choice); a sliced view that starts elsewhere moves row by row.
template <typename T, int R>
using Pack = T __attribute__((ext_vector_type(R)));
__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <typename T, int R>
__device__ __forceinline__ void load_pack(const T* p, int64_t row0, int cnt, T (&v)[R])
{
  static_assert(sizeof(T) * R == 16, "one access is 16 bytes");
  if (cnt == R && aligned16(p)) {
    const Pack<T, R> pk = *reinterpret_cast<const Pack<T, R>*>(p + row0);
#pragma unroll
    for (int k = 0; k < R; ++k) v[k] = pk[k];
  } else {
#pragma unroll
    for (int k = 0; k < R; ++k) {
      v[k] = T(0);
      if (k < cnt) v[k] = p[row0 + k];
    }
  }
}
template <typename T, int R>
__device__ __forceinline__ void store_pack(T* p, int64_t row0, int cnt, const T (&v)[R])
{
  if (cnt == R && aligned16(p)) {
    Pack<T, R> pk;
#pragma unroll
    for (int k = 0; k < R; ++k) pk[k] = v[k];
    *reinterpret_cast<Pack<T, R>*>(p + row0) = pk;
  } else {
#pragma unroll
    for (int k = 0; k < R; ++k)
      if (k < cnt) p[row0 + k] = v[k];
  }
}
// a column's R rows from row0 on, or R copies of a scalar
template <typename T, int R>
__device__ __forceinline__ void load_src(const ValueSrc& s, int64_t row0, int cnt, T (&v)[R])
{
  const T* p = static_cast<const T*>(s.data);
  if (s.is_scalar) {
    const T x = p[0];
#pragma unroll
    for (int k = 0; k < R; ++k) v[k] = x;
  } else {
    load_pack<T, R>(p, row0, cnt, v);
  }
}
// the validity of the cnt (0..16) rows of a thread from row0 on
__device__ __forceinline__ uint32_t src_bits(const ValueSrc& s, int64_t row0, int cnt, bool scalar_ok)
{
  if (cnt <= 0) return 0u;
  return s.valid ? bits_from(s.valid, s.begin_bit + row0, cnt) : (scalar_ok ? low_mask32(cnt) : 0u);
}

// The threads of a tile: access j of thread t covers the R rows from (j * 256 + t) * R of the tile on, so a wave's access is one
// contiguous run of 64 * R rows.  f(row0, cnt) is called by EVERY lane of a wave that has a live row in the access (cnt = 0 for
// the lanes behind the last row), which is what store_thread_bits needs.
template <int R, typename F>
__device__ __forceinline__ void for_each_access(int64_t n, F&& f)
{
  const unsigned lane = lane_id();
  const int64_t tiles = div_up(n, TILE);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
#pragma unroll 1
    for (int j = 0; j < ROWS / R; ++j) {
      const int64_t row0 = tile * TILE + ((int64_t)j * BT + threadIdx.x) * R;
      if (row0 - (int64_t)lane * R >= n) break;  // the whole wave is behind the last row, in this access and in the later ones
      f(row0, row0 >= n ? 0 : (n - row0 < R ? (int)(n - row0) : R));
    }
  }
}
// The R validity bits of a thread's rows (0 for rows at and behind n) into the output bitmap: the 32 / R lanes that share a word
// merge their bits across the wave and the first of them writes the word -- k_elementwise's merge: one writer per word, every
// word below (n + 31) / 32 written, bits behind the last row 0.  Every lane of the wave must call it.
template <int R>
__device__ __forceinline__ void store_thread_bits(uint32_t* __restrict__ out_valid, int64_t row0, int64_t n, uint32_t ob)
{
  constexpr int GROUP = 32 / R;
  const unsigned lane = lane_id();
  uint32_t w          = ob << ((lane % GROUP) * R);
#pragma unroll
  for (int d = 1; d < GROUP; d <<= 1) w |= (uint32_t)__shfl_xor((int)w, d, GX_WAVE);
  if (lane % GROUP == 0 && row0 < n) out_valid[row0 >> 5] = w;
}

// ---------------------------------------------------------------- replace_nulls with a column or a scalar
template <typename T>
__global__ void __launch_bounds__(BT) k_replace_nulls(ValueSrc in, ValueSrc repl, int64_t n, T* __restrict__ out,
                                                      uint32_t* __restrict__ out_valid, unsigned long long* __restrict__ null_count)
{
  constexpr int R = 16 / (int)sizeof(T);
  __shared__ unsigned long long s_nulls;
  const bool r_ok = repl.scalar_ok();
  if (null_count) tally_begin(&s_nulls);
  unsigned long long nulls = 0;
  for_each_access<R>(n, [&](int64_t row0, int cnt) {
    const uint32_t lm = low_mask32(cnt);
    const uint32_t ib = src_bits(in, row0, cnt, true), rb = src_bits(repl, row0, cnt, r_ok);
    if (cnt > 0) {
      T x[R];
      load_src<T, R>(in, row0, cnt, x);
      if (ib != lm) {  // the replacement is read only where a row needs it
        T y[R];
        load_src<T, R>(repl, row0, cnt, y);
#pragma unroll
        for (int k = 0; k < R; ++k) x[k] = (ib >> k) & 1u ? x[k] : y[k];
      }
      store_pack<T, R>(out, row0, cnt, x);
    }
    if (out_valid) {
      const uint32_t ob = (ib | rb) & lm;
      store_thread_bits<R>(out_valid, row0, n, ob);
      nulls += (unsigned long long)__builtin_popcount(~ob & lm);
    }
  });
  if (null_count) tally_end(&s_nulls, wave_reduce(nulls, SumOp()), null_count);
}

// ---------------------------------------------------------------- replace_nans
template <typename T>
__global__ void __launch_bounds__(BT) k_replace_nans(ValueSrc in, ValueSrc repl, int64_t n, T* __restrict__ out,
                                                     uint32_t* __restrict__ out_valid, unsigned long long* __restrict__ null_count)
{
  constexpr int R = 16 / (int)sizeof(T);
  __shared__ unsigned long long s_nulls;
  const bool r_ok = repl.scalar_ok();
  if (null_count) tally_begin(&s_nulls);
  unsigned long long nulls = 0;
  for_each_access<R>(n, [&](int64_t row0, int cnt) {
    const uint32_t lm = low_mask32(cnt);
    const uint32_t ib = src_bits(in, row0, cnt, true), rb = src_bits(repl, row0, cnt, r_ok);
    uint32_t take = 0;  // valid rows that hold a NaN
    if (cnt > 0) {
      T x[R];
      load_src<T, R>(in, row0, cnt, x);
#pragma unroll
      for (int k = 0; k < R; ++k) take |= (x[k] != x[k] ? 1u : 0u) << k;
      take &= ib;
      if (take) {
        T y[R];
        load_src<T, R>(repl, row0, cnt, y);
#pragma unroll
        for (int k = 0; k < R; ++k) x[k] = (take >> k) & 1u ? y[k] : x[k];
      }
      store_pack<T, R>(out, row0, cnt, x);
    }
    if (out_valid) {
      const uint32_t ob = ((ib & ~take) | (take & rb)) & lm;
      store_thread_bits<R>(out_valid, row0, n, ob);
      nulls += (unsigned long long)__builtin_popcount(~ob & lm);
    }
  });
  if (null_count) tally_end(&s_nulls, wave_reduce(nulls, SumOp()), null_count);
}

// ---------------------------------------------------------------- clamp
// T is the column's own type (BOOL8: uint8_t with ISBOOL, compared as x != 0; a row inside the bounds keeps its byte)
template <typename T, bool ISBOOL>
__global__ void __launch_bounds__(BT) k_clamp(const T* __restrict__ in, int64_t n, const T* __restrict__ lo, const uint8_t* __restrict__ lo_valid,
                                              const T* __restrict__ lo_replace, const T* __restrict__ hi, const uint8_t* __restrict__ hi_valid,
                                              const T* __restrict__ hi_replace, T* __restrict__ out)
{
  constexpr int R   = 16 / (int)sizeof(T);
  const bool has_lo = lo && (!lo_valid || *lo_valid != 0);
  const bool has_hi = hi && (!hi_valid || *hi_valid != 0);
  T lo_v = T(0), hi_v = T(0), lo_r = T(0), hi_r = T(0);
  if (has_lo) {
    lo_v = *lo;
    lo_r = lo_replace ? *lo_replace : lo_v;
  }
  if (has_hi) {
    hi_v = *hi;
    hi_r = hi_replace ? *hi_replace : hi_v;
  }
  if (ISBOOL) {
    lo_v = T(lo_v != T(0));
    hi_v = T(hi_v != T(0));
    lo_r = T(lo_r != T(0));
    hi_r = T(hi_r != T(0));
  }
  for_each_access<R>(n, [&](int64_t row0, int cnt) {
    if (cnt == 0) return;
    T x[R];
    load_pack<T, R>(in, row0, cnt, x);
#pragma unroll
    for (int k = 0; k < R; ++k) {
      const T c = ISBOOL ? T(x[k] != T(0)) : x[k];
      if (has_lo && c < lo_v) x[k] = lo_r;
      else if (has_hi && c > hi_v) x[k] = hi_r;
    }
    store_pack<T, R>(out, row0, cnt, x);
  });
}

// ---------------------------------------------------------------- find_and_replace
// T: the unsigned type of the element's width for integers and BOOL8 (== is the equality of the bits), float / double for floats
// (NaN matches nothing, -0.0 matches +0.0).  A thread keeps its 16 rows of the tile in registers while the workgroup walks the
// list of old values through LDS, FR_CHUNK at a time; a row takes the first index that matches and keeps it.
template <typename T>
__global__ void __launch_bounds__(BT) k_find_replace(const T* __restrict__ in, const uint32_t* __restrict__ in_valid, int64_t in_begin_bit,
                                                     int64_t n, const T* __restrict__ old_vals, const T* __restrict__ new_vals,
                                                     const uint32_t* __restrict__ new_valid, int64_t new_begin_bit, int64_t m,
                                                     T* __restrict__ out, uint32_t* __restrict__ out_valid,
                                                     unsigned long long* __restrict__ null_count)
{
  constexpr int R  = 16 / (int)sizeof(T);
  constexpr int NJ = ROWS / R;
  __shared__ T s_old[FR_CHUNK];
  __shared__ unsigned long long s_nulls;
  if (null_count) tally_begin(&s_nulls);
  unsigned long long nulls = 0;
  const int64_t tiles      = div_up(n, TILE);
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {  // (workgroup-uniform: every thread meets the barriers)
    T x[ROWS];
    int32_t idx[ROWS];
    uint32_t ib[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int64_t row0 = tile * TILE + ((int64_t)j * BT + threadIdx.x) * R;
      const int cnt      = row0 >= n ? 0 : (n - row0 < R ? (int)(n - row0) : R);
      T v[R];
#pragma unroll
      for (int k = 0; k < R; ++k) v[k] = T(0);
      if (cnt > 0) load_pack<T, R>(in, row0, cnt, v);
      ib[j] = cnt > 0 ? (in_valid ? bits_from(in_valid, in_begin_bit + row0, cnt) : low_mask32(cnt)) : 0u;
#pragma unroll
      for (int k = 0; k < R; ++k) {
        x[j * R + k]   = v[k];
        idx[j * R + k] = (ib[j] >> k) & 1u ? -1 : -2;  // -1: still looking; -2: a null row (or none), not compared
      }
    }
    for (int64_t c0 = 0; c0 < m; c0 += FR_CHUNK) {
      const int len = m - c0 < FR_CHUNK ? (int)(m - c0) : FR_CHUNK;
      __syncthreads();  // the chunk before this one has been read by everyone
      for (int i = threadIdx.x; i < len; i += BT) s_old[i] = old_vals[c0 + i];
      __syncthreads();
      for (int jj = 0; jj < len; ++jj) {
        const T ov = s_old[jj];  // one address for the whole wave: an LDS broadcast
#pragma unroll
        for (int k = 0; k < ROWS; ++k)
          if (idx[k] == -1 && x[k] == ov) idx[k] = (int32_t)(c0 + jj);
      }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int64_t row0 = tile * TILE + ((int64_t)j * BT + threadIdx.x) * R;
      const int cnt      = row0 >= n ? 0 : (n - row0 < R ? (int)(n - row0) : R);
      uint32_t ob        = ib[j];
      T v[R];
#pragma unroll
      for (int k = 0; k < R; ++k) {
        v[k]            = x[j * R + k];
        const int32_t f = idx[j * R + k];
        if (f >= 0) {
          v[k] = new_vals[f];
          if (new_valid && !bit_is_set(new_valid, new_begin_bit + f)) ob &= ~(1u << k);
        }
      }
      if (cnt > 0) store_pack<T, R>(out, row0, cnt, v);
      if (out_valid) {  // every lane of the wave is here
        store_thread_bits<R>(out_valid, row0, n, ob);
        nulls += (unsigned long long)__builtin_popcount(~ob & low_mask32(cnt));
      }
    }
  }
  if (null_count) tally_end(&s_nulls, wave_reduce(nulls, SumOp()), null_count);
}

// ---------------------------------------------------------------- normalize_nans_and_zeros
// U: the bits of a float / double.  out may be in: a thread reads its rows before it writes the same rows.
template <typename U>
__global__ void __launch_bounds__(BT) k_normalize(const U* in, int64_t n, U* out)
{
  constexpr int R  = 16 / (int)sizeof(U);
  constexpr U SIGN = U(U(1) << (sizeof(U) * 8 - 1));
  constexpr U EXP  = sizeof(U) == 8 ? U(0x7FF0000000000000ull) : U(0x7F800000u);
  constexpr U QNAN = sizeof(U) == 8 ? U(0x7FF8000000000000ull) : U(0x7FC00000u);
  for_each_access<R>(n, [&](int64_t row0, int cnt) {
    if (cnt == 0) return;
    U x[R];
    load_pack<U, R>(in, row0, cnt, x);
#pragma unroll
    for (int k = 0; k < R; ++k) {
      if (U(x[k] & U(~SIGN)) > EXP) x[k] = QNAN;
      else if (x[k] == SIGN) x[k] = U(0);
    }
    store_pack<U, R>(out, row0, cnt, x);
  });
}

// ---------------------------------------------------------------- replace_nulls with a policy
// The source row of a null is a function of the bitmap alone, so no workgroup waits for another:
//   1. k_tile_table: per tile, the valid row of the tile nearest to the tiles behind it in fill direction, as a KEY, or -1;
//   2. k_carry_local / k_carry_top: an exclusive running max over that table, in two levels of fixed depth;
//   3. k_policy_fill: a tile resolves every null inside itself and takes the carried row where it has no source of its own.
// Both directions are one computation through the key: PRECEDING key = row, entry = tile; FOLLOWING key = n - 1 - row, entry =
// tiles - 1 - tile.  The nearest valid row strictly before (after) a tile is then the largest key of the entries below its own.
__device__ __forceinline__ uint64_t span_bits(const uint32_t* __restrict__ valid, int64_t begin_bit, int64_t r0, int64_t n)
{
  if (r0 >= n) return 0ull;
  const int64_t end = r0 + 64 < n ? r0 + 64 : n;
  return bits_from64(valid, begin_bit + r0, begin_bit + end);
}

// one wave per tile, one 64-row span per lane
template <bool BACK>
__global__ void __launch_bounds__(BT) k_tile_table(const uint32_t* __restrict__ valid, int64_t begin_bit, int64_t n, int64_t tiles,
                                                   int32_t* __restrict__ table)
{
  const unsigned lane  = lane_id();
  const int64_t stride = (int64_t)gridDim.x * (BT / GX_WAVE);
  for (int64_t tile = (int64_t)blockIdx.x * (BT / GX_WAVE) + threadIdx.x / GX_WAVE; tile < tiles; tile += stride) {
    const int64_t r0 = tile * TILE + 64 * (int64_t)lane;
    const uint64_t b = span_bits(valid, begin_bit, r0, n);
    int32_t key      = -1;
    if (b) key = BACK ? (int32_t)(n - 1 - (r0 + __builtin_ctzll(b))) : (int32_t)(r0 + 63 - __builtin_clzll(b));
    key = wave_reduce(key, MaxOp());
    if (lane == 0) table[BACK ? tiles - 1 - tile : tile] = key;
  }
}

// table[e] becomes the largest key of the entries of e's block below e (-1: none), top[block] the largest key of the block
__global__ void __launch_bounds__(BT) k_carry_local(int32_t* __restrict__ table, int64_t tiles, int32_t* __restrict__ top)
{
  constexpr int PER = CARRY_BLOCK / BT;
  __shared__ int32_t lds[BT / GX_WAVE + 1];
  const int64_t e0 = (int64_t)blockIdx.x * CARRY_BLOCK + (int64_t)threadIdx.x * PER;
  int32_t v[PER];
  int32_t mine = -1;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    v[k] = e0 + k < tiles ? table[e0 + k] : -1;
    mine = v[k] > mine ? v[k] : mine;
  }
  int32_t total;
  int32_t run = block_exclusive_scan<BT>(mine, (int32_t)-1, MaxOp(), lds, &total);
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    if (e0 + k < tiles) table[e0 + k] = run;
    run = v[k] > run ? v[k] : run;
  }
  if (threadIdx.x == 0) top[blockIdx.x] = total;
}
// top[b] becomes the largest key of the blocks below b: one workgroup, at most 2^31 / (TILE * CARRY_BLOCK) = 512 blocks
constexpr int TOP_BT = 512;
static_assert((int64_t(1) << 31) / ((int64_t)TILE * CARRY_BLOCK) <= TOP_BT, "the top level is one block scan without a loop");
__global__ void __launch_bounds__(TOP_BT) k_carry_top(int32_t* __restrict__ top, int blocks)
{
  __shared__ int32_t lds[TOP_BT / GX_WAVE + 1];
  const int32_t v   = (int)threadIdx.x < blocks ? top[threadIdx.x] : -1;
  const int32_t run = block_exclusive_scan<TOP_BT>(v, (int32_t)-1, MaxOp(), lds, (int32_t*)nullptr);
  if ((int)threadIdx.x < blocks) top[threadIdx.x] = run;
}

// A tile: wave 0 reads the tile's 64 validity spans, one per lane, and scans, in fill direction, the nearest valid row up to and
// including each span into the per-word table s_near (tile-relative keys).  Then a wave takes a span at a time, a row per lane:
// a null row finds its source in its own span from the span's bits (clz / ctz below / above its lane), else in s_near of the
// neighbouring span, else it is the tile's carried row.  A row is ONE load, in[source], the row itself where it is valid -- the
// sources of a tile lie in the tile, which streams through the caches once, or are the one carried row -- and one store.
template <typename T, bool BACK>
__global__ void __launch_bounds__(BT) k_policy_fill(const T* __restrict__ in, const uint32_t* __restrict__ valid, int64_t begin_bit, int64_t n,
                                                    int64_t tiles, const int32_t* __restrict__ carry_local, const int32_t* __restrict__ carry_top,
                                                    T* __restrict__ out, uint32_t* __restrict__ out_valid,
                                                    unsigned long long* __restrict__ null_count)
{
  __shared__ uint64_t s_bits[WORDS];
  __shared__ int32_t s_near[WORDS];
  __shared__ unsigned long long s_nulls;
  const unsigned lane = lane_id();
  const unsigned wave = threadIdx.x / GX_WAVE;
  if (null_count) tally_begin(&s_nulls);
  unsigned long long nulls = 0;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t t0 = tile * TILE;
    if (wave == 0) {
      const int w      = BACK ? WORDS - 1 - (int)lane : (int)lane;  // lanes in fill direction
      const uint64_t b = span_bits(valid, begin_bit, t0 + 64 * (int64_t)w, n);
      int32_t key      = -1;
      if (b) key = BACK ? TILE - 1 - (64 * w + __builtin_ctzll(b)) : 64 * w + 63 - __builtin_clzll(b);
      s_bits[w] = b;
      s_near[w] = wave_inclusive_scan(key, MaxOp());
    }
    // the row carried into this tile: the nearest valid row of the tiles behind it in fill direction (workgroup-uniform)
    const int64_t e = BACK ? tiles - 1 - tile : tile;
    int32_t ckey    = carry_local[e];
    const int32_t tk = carry_top[e / CARRY_BLOCK];
    ckey            = tk > ckey ? tk : ckey;
    const int64_t carry_row = ckey < 0 ? -1 : (BACK ? n - 1 - ckey : (int64_t)ckey);
    __syncthreads();
    for (int sp = (int)wave; sp < WORDS; sp += BT / GX_WAVE) {
      const int64_t r0 = t0 + 64 * (int64_t)sp;
      if (r0 >= n) break;  // wave-uniform
      const int64_t r  = r0 + lane;
      const uint64_t b = s_bits[sp];
      int64_t src      = r;
      if (!((b >> lane) & 1u)) {
        if (BACK) {
          const uint64_t above = b & ~low_mask64((int)lane + 1);
          const int32_t k      = sp + 1 < WORDS ? s_near[sp + 1] : -1;
          src = above ? r0 + __builtin_ctzll(above) : (k >= 0 ? t0 + (TILE - 1 - k) : carry_row);
        } else {
          const uint64_t below = b & low_mask64((int)lane);
          const int32_t k      = sp > 0 ? s_near[sp - 1] : -1;
          src = below ? r0 + 63 - __builtin_clzll(below) : (k >= 0 ? t0 + k : carry_row);
        }
      }
      const bool has = r < n && src >= 0;
      if (has) out[r] = in[src];
      const uint64_t ob = store_wave_validity(out_valid, r0, n, has);
      nulls += (unsigned long long)((n - r0 < 64 ? (int)(n - r0) : 64) - __builtin_popcountll(ob));  // (wave-uniform)
    }
    __syncthreads();  // the tables are rewritten for the next tile
  }
  if (null_count) tally_end(&s_nulls, nulls, null_count);
}

static inline unsigned tile_grid(int64_t n) { return capped_grid(n, TILE, GRID_CAP); }

}  // namespace rp
}  // namespace gx

extern "C" {

int gx_replace_tile_rows(void) { return gx::rp::TILE; }
int gx_find_and_replace_chunk(void) { return gx::rp::FR_CHUNK; }

int gx_replace_nulls(int elem_size, const void* in, const uint32_t* in_valid, int64_t in_begin_bit, const void* repl,
                     const uint32_t* repl_valid, int64_t repl_begin_bit, const uint8_t* repl_scalar_valid_dev, int repl_is_scalar,
                     int64_t n, void* out, uint32_t* out_valid, int64_t* out_null_count_dev, gx_stream_t s)
{
  using namespace gx::rp;
  if (!width_ok(elem_size)) return GX_EDTYPE;
  if (n < 0 || n > MAX_ROWS || in_begin_bit < 0 || repl_begin_bit < 0) return GX_EINVAL;
  if (n == 0) return 0;
  if (!in || !repl || !out) return GX_EINVAL;
  if (out_null_count_dev) GX_HIP_TRY(hipMemsetAsync(out_null_count_dev, 0, sizeof(int64_t), s));
  const gx::ValueSrc i{in, in_valid, in_begin_bit, nullptr, 0};
  const gx::ValueSrc r{repl, repl_is_scalar ? nullptr : repl_valid, repl_begin_bit, repl_scalar_valid_dev, repl_is_scalar};
  unsigned long long* nulls = out_valid ? reinterpret_cast<unsigned long long*>(out_null_count_dev) : nullptr;
  return gx::with_width(elem_size, [&](auto tag) {
    using T = decltype(tag);
    hipLaunchKernelGGL((k_replace_nulls<T>), dim3(tile_grid(n)), dim3(BT), 0, s, i, r, n, static_cast<T*>(out), out_valid, nulls);
    GX_LAUNCH_CHECK();
    return 0;
  });
}

int gx_replace_nulls_policy(int elem_size, const void* in, const uint32_t* in_valid, int64_t in_begin_bit, int64_t n, int backward,
                            void* out, uint32_t* out_valid, int64_t* out_null_count_dev, void* tmp, size_t* tmp_bytes, gx_stream_t s)
{
  using namespace gx::rp;
  if (!width_ok(elem_size)) return GX_EDTYPE;
  if (n < 0 || n > MAX_ROWS || in_begin_bit < 0 || !tmp_bytes) return GX_EINVAL;
  const int64_t tiles  = gx::div_up(n, TILE);
  const int64_t blocks = gx::div_up(tiles, CARRY_BLOCK);
  gx::Carver cv(tmp);
  int32_t* table = cv.take<int32_t>((size_t)tiles);
  int32_t* top   = cv.take<int32_t>((size_t)blocks);
  if (int rc; !cv.ready(tmp_bytes, &rc)) return rc;
  if (n == 0) return 0;
  if (!in || !in_valid || !out || !out_valid) return GX_EINVAL;
  if (out_null_count_dev) GX_HIP_TRY(hipMemsetAsync(out_null_count_dev, 0, sizeof(int64_t), s));
  const unsigned table_grid = gx::capped_grid(tiles, BT / GX_WAVE, GRID_CAP);
  if (backward)
    hipLaunchKernelGGL((k_tile_table<true>), dim3(table_grid), dim3(BT), 0, s, in_valid, in_begin_bit, n, tiles, table);
  else
    hipLaunchKernelGGL((k_tile_table<false>), dim3(table_grid), dim3(BT), 0, s, in_valid, in_begin_bit, n, tiles, table);
  hipLaunchKernelGGL(k_carry_local, dim3((unsigned)blocks), dim3(BT), 0, s, table, tiles, top);
  hipLaunchKernelGGL(k_carry_top, dim3(1), dim3(TOP_BT), 0, s, top, (int)blocks);
  GX_LAUNCH_CHECK();
  unsigned long long* nulls = reinterpret_cast<unsigned long long*>(out_null_count_dev);
  return gx::with_width(elem_size, [&](auto tag) {
    using T = decltype(tag);
    if (backward)
      hipLaunchKernelGGL((k_policy_fill<T, true>), dim3(tile_grid(n)), dim3(BT), 0, s, static_cast<const T*>(in), in_valid, in_begin_bit, n,
                         tiles, table, top, static_cast<T*>(out), out_valid, nulls);
    else
      hipLaunchKernelGGL((k_policy_fill<T, false>), dim3(tile_grid(n)), dim3(BT), 0, s, static_cast<const T*>(in), in_valid, in_begin_bit, n,
                         tiles, table, top, static_cast<T*>(out), out_valid, nulls);
    GX_LAUNCH_CHECK();
    return 0;
  });
}

int gx_replace_nans(int dtype, const void* in, const uint32_t* in_valid, int64_t in_begin_bit, const void* repl,
                    const uint32_t* repl_valid, int64_t repl_begin_bit, const uint8_t* repl_scalar_valid_dev, int repl_is_scalar, int64_t n,
                    void* out, uint32_t* out_valid, int64_t* out_null_count_dev, gx_stream_t s)
{
  using namespace gx::rp;
  if (!is_float(dtype)) return GX_EDTYPE;
  if (n < 0 || n > MAX_ROWS || in_begin_bit < 0 || repl_begin_bit < 0) return GX_EINVAL;
  if (n == 0) return 0;
  if (!in || !repl || !out) return GX_EINVAL;
  const bool repl_nullable = repl_is_scalar ? repl_scalar_valid_dev != nullptr : repl_valid != nullptr;
  if (!out_valid && (in_valid || repl_nullable)) return GX_EINVAL;  // a side that can be null needs a bitmap to say so
  if (out_null_count_dev) GX_HIP_TRY(hipMemsetAsync(out_null_count_dev, 0, sizeof(int64_t), s));
  const gx::ValueSrc i{in, in_valid, in_begin_bit, nullptr, 0};
  const gx::ValueSrc r{repl, repl_is_scalar ? nullptr : repl_valid, repl_begin_bit, repl_scalar_valid_dev, repl_is_scalar};
  unsigned long long* nulls = out_valid ? reinterpret_cast<unsigned long long*>(out_null_count_dev) : nullptr;
  if (dtype == GX_FLOAT32)
    hipLaunchKernelGGL((k_replace_nans<float>), dim3(tile_grid(n)), dim3(BT), 0, s, i, r, n, static_cast<float*>(out), out_valid, nulls);
  else
    hipLaunchKernelGGL((k_replace_nans<double>), dim3(tile_grid(n)), dim3(BT), 0, s, i, r, n, static_cast<double*>(out), out_valid, nulls);
  GX_LAUNCH_CHECK();
  return 0;
}

int gx_clamp(int dtype, const void* in, int64_t n, const void* lo, const uint8_t* lo_valid_dev, const void* lo_replace, const void* hi,
             const uint8_t* hi_valid_dev, const void* hi_replace, void* out, gx_stream_t s)
{
  using namespace gx::rp;
  if (n < 0 || n > MAX_ROWS) return GX_EINVAL;
  if (!dtype_ok(dtype)) return GX_EDTYPE;
  if (n == 0) return 0;
  if (!in || !out) return GX_EINVAL;
  return gx::with_dtype(dtype, [&](auto t) {
    using D = decltype(t);
    using T = typename D::value_type;
    hipLaunchKernelGGL((k_clamp<T, D::is_bool>), dim3(tile_grid(n)), dim3(BT), 0, s, static_cast<const T*>(in), n, static_cast<const T*>(lo),
                       lo_valid_dev, static_cast<const T*>(lo_replace), static_cast<const T*>(hi), hi_valid_dev,
                       static_cast<const T*>(hi_replace), static_cast<T*>(out));
    GX_LAUNCH_CHECK();
    return 0;
  });
}

int gx_find_and_replace(int dtype, const void* in, const uint32_t* in_valid, int64_t in_begin_bit, int64_t n, const void* old_vals,
                        const void* new_vals, const uint32_t* new_valid, int64_t new_begin_bit, int64_t m, void* out, uint32_t* out_valid,
                        int64_t* out_null_count_dev, gx_stream_t s)
{
  using namespace gx::rp;
  if (n < 0 || n > MAX_ROWS || m < 0 || m > MAX_ROWS || in_begin_bit < 0 || new_begin_bit < 0) return GX_EINVAL;
  if (!dtype_ok(dtype)) return GX_EDTYPE;
  if (n == 0) return 0;
  if (!in || !out || (m > 0 && (!old_vals || !new_vals))) return GX_EINVAL;
  if (!out_valid && (in_valid || (m > 0 && new_valid))) return GX_EINVAL;
  if (out_null_count_dev) GX_HIP_TRY(hipMemsetAsync(out_null_count_dev, 0, sizeof(int64_t), s));
  unsigned long long* nulls = out_valid ? reinterpret_cast<unsigned long long*>(out_null_count_dev) : nullptr;
  return gx::with_dtype(dtype, [&](auto t) {  // integers match by their bits whatever their sign, floats by value
    using T = gx::word_or_float_t<decltype(t)>;
    hipLaunchKernelGGL((k_find_replace<T>), dim3(tile_grid(n)), dim3(BT), 0, s, static_cast<const T*>(in), in_valid, in_begin_bit, n,
                       static_cast<const T*>(old_vals), static_cast<const T*>(new_vals), new_valid, new_begin_bit, m, static_cast<T*>(out),
                       out_valid, nulls);
    GX_LAUNCH_CHECK();
    return 0;
  });
}

int gx_normalize_nans_and_zeros(int dtype, const void* in, int64_t n, void* out, gx_stream_t s)
{
  using namespace gx::rp;
  if (!is_float(dtype)) return GX_EDTYPE;
  if (n < 0 || n > MAX_ROWS) return GX_EINVAL;
  if (n == 0) return 0;
  if (!in || !out) return GX_EINVAL;
  if (dtype == GX_FLOAT32)
    hipLaunchKernelGGL((k_normalize<uint32_t>), dim3(tile_grid(n)), dim3(BT), 0, s, static_cast<const uint32_t*>(in), n, static_cast<uint32_t*>(out));
  else
    hipLaunchKernelGGL((k_normalize<uint64_t>), dim3(tile_grid(n)), dim3(BT), 0, s, static_cast<const uint64_t*>(in), n, static_cast<uint64_t*>(out));
  GX_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
