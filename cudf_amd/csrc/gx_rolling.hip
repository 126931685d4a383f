// gx_rolling.hip -- rolling-window aggregations: the kernels behind cudf::rolling_window / grouped_rolling_window
// (include/cudf/rolling.hpp).  Replaces the reference's one-thread-per-row window loop (rolling_detail.cuh) on its fixed-window path.
//
// Window of row i: rows [i - preceding + 1, i + following], cut to [0, n), or to the row's group [offsets[g], offsets[g + 1]).
// Everything about a window is computed in 64 bits.  SUM / MIN / MAX / MEAN / COUNT_VALID / COUNT_ALL; the rules are in gx.h.
//
// Accumulators (the form an element takes in LDS and in the row loop):
//   M_ISUM  integers and BOOL8, SUM / MEAN: the element widened to 64 bits, added mod 2^64
//   M_FSUM  floats, SUM / MEAN: double, plain addition (inf, NaN and overflow are what the additions give)
//   M_MIN   MIN / MAX of every type: the element's 64-bit SORTABLE key (signed: sign flip; float: widened to double, -0.0 -> +0.0,
//           NaN -> all ones, IEEE total-order flip: gx_common.hpp to_sortable), MAX on the inverted key, so one unsigned minimum
//           serves both and NaN is greater than every number
//   M_COUNT the counts: no value at all
// A null is the accumulator's identity and a valid count of 0; its bytes are not read.
//
// k_roll_tile (fixed windows, L = preceding + following >= 1, halo = max(preceding - 1, 0) + max(following, 0) <= SPAN): one
//   workgroup per TILE output rows.
//   A  the region [tile_lo - left halo, tile_hi + right halo] is read once, coalesced, into LDS as accumulators, with a flag byte
//      per row (first row of its group, last row of its group, valid).  Rows outside [0, n) are identities that start and end a group.
//   B  every thread takes ITEMS consecutive region rows into registers.  Each group is cut into segments of L rows from its first
//      row; a forward scan that restarts at every segment head and a backward scan that restarts at every segment tail (the last
//      row of a segment or of the group) are computed: the thread's rows serially, the thread aggregates by a segmented wave64
//      scan (gx_common.hpp wave_inclusive_scan on (restart, value, count)), the four wave aggregates through LDS.  The position
//      of a row inside its segment is divided out once per thread and counted from there.
//   C  the cut window [lo, hi] of an output row holds at most L rows, so it touches at most two segments:
//        lo and hi in different segments   suffix[lo] (op) prefix[hi]
//        lo a segment head                 prefix[hi]
//        otherwise (hi is a tail)          suffix[lo]
//      Two LDS reads and one operation per row whatever L is -- and no subtraction: a difference of prefix sums would cancel on
//      floats and carry one inf into every later window.  The valid counts ride the same scans (16-bit: a region has <= 4352
//      rows); without a bitmap the count is hi - lo + 1.
//   LDS image: row k of the region sits at k + k / ITEMS, ITEMS even, so a thread's run starts ITEMS + 1 (odd) elements after its
//   neighbour's: the 8-byte reads and writes of phase B, stride 2 * (ITEMS + 1) dwords, fall on 32 distinct even banks per 32 lanes.
// k_roll_rows (per-row window columns, halo > SPAN, L <= 0, and by default L <= DIRECT_MAX): one row per thread, a loop over its cut
//   window from global memory: O(window) per row.
// Validity: a wave writes the two bitmap words of its 64 rows; the null count is counted from the finished bitmap afterwards.
#include "gx_common.hpp"

#include <type_traits>

namespace gx {
namespace roll {

constexpr int BT   = 256;   // threads of a workgroup
constexpr int TILE = 2048;  // output rows per workgroup
constexpr int SPAN = 2048;  // largest halo the tile kernel takes: at most (TILE + SPAN) / BT = 16 region rows per thread
constexpr int NWV  = BT / GX_WAVE;
// the default choice (gx_rolling_set_kernel(0)): windows of up to DIRECT_MAX rows take the row loop, which re-reads its few rows from
// the caches faster than the tile kernel stages them (xp_rolling, 2^28 rows: L = 2 1.21 against 2.33 ms, L = 8 1.88 against 2.33 ms,
// with a bitmap 2.99 against 4.09, in groups 2.53 against 3.95; at L = 64 it loses 8.4 against 2.35): DESIGN.md, rolling windows
constexpr int DIRECT_MAX = 8;

enum Mode { M_ISUM = 0, M_FSUM = 1, M_MIN = 2, M_COUNT = 3 };
enum OutKind { O_BITS64, O_F32, O_F64, O_MEAN_I, O_MEAN_U, O_MEAN_F, O_KEY, O_COUNT_VALID, O_COUNT_ALL };
enum Flag : uint8_t { F_START = 1, F_END = 2, F_VALID = 4 };

struct Args {
  const void* in;
  const uint32_t* valid;
  int64_t bit0, n;
  int64_t p, f;                 // the fixed window (clamped to +-2^31 by the host: every such window is empty or whole anyway)
  const int32_t *pcol, *fcol;   // or one window per row
  const int32_t *labels, *offsets;
  int min_periods, dtype, out_kind;
  uint64_t inv;                 // M_MIN: 0 for MIN, ~0 for MAX
  void* out;
  uint32_t* out_valid;
};

template <typename F>
__device__ __forceinline__ void with_type(int dtype, F&& f)
{
  switch (dtype) {
    case GX_INT8: f(int8_t{}); break;
    case GX_INT16: f(int16_t{}); break;
    case GX_INT32: f(int32_t{}); break;
    case GX_INT64: f(int64_t{}); break;
    case GX_UINT8:
    case GX_BOOL8: f(uint8_t{}); break;
    case GX_UINT16: f(uint16_t{}); break;
    case GX_UINT32: f(uint32_t{}); break;
    case GX_UINT64: f(uint64_t{}); break;
    case GX_FLOAT32: f(float{}); break;
    default: f(double{}); break;
  }
}

template <int MODE>
struct Acc {
  using type = uint64_t;
};
template <>
struct Acc<M_FSUM> {
  using type = double;
};

template <int MODE>
__device__ __forceinline__ typename Acc<MODE>::type identity()
{
  if constexpr (MODE == M_MIN) return ~0ull;
  else return typename Acc<MODE>::type(0);
}
template <int MODE, typename A>
__device__ __forceinline__ A combine(A a, A b)
{
  if constexpr (MODE == M_MIN) return b < a ? b : a;
  else return a + b;
}

template <int MODE, typename T>
__device__ __forceinline__ typename Acc<MODE>::type to_acc(T x, uint64_t inv)
{
  if constexpr (MODE == M_FSUM) {
    return (double)x;
  } else if constexpr (MODE == M_ISUM) {
    if constexpr (std::is_floating_point<T>::value) return 0;  // (not dispatched)
    else if constexpr (std::is_signed<T>::value) return (uint64_t)(int64_t)x;
    else return (uint64_t)x;
  } else if constexpr (MODE == M_MIN) {
    uint64_t key;
    if constexpr (std::is_floating_point<T>::value) {
      const double d = (double)x;
      uint64_t bits;
      __builtin_memcpy(&bits, &d, 8);
      key = to_sortable<uint64_t, K_FLOAT>(bits, 0);
    } else if constexpr (std::is_signed<T>::value) {
      key = (uint64_t)(int64_t)x ^ 0x8000000000000000ull;
    } else {
      key = (uint64_t)x;
    }
    return key ^ inv;
  } else {
    return 0;
  }
}

// [gs, ge) of row i
__device__ __forceinline__ void group_of(const Args& a, int64_t i, int64_t& gs, int64_t& ge)
{
  gs = 0;
  ge = a.n;
  if (a.labels) {
    const int32_t g = a.labels[i];
    gs              = a.offsets[g];
    ge              = a.offsets[g + 1];
  }
}

// the result of row i: `value` over `cnt` valid values of a cut window of `size` rows.  Returns the row's validity.
template <int MODE>
__device__ __forceinline__ bool store_row(const Args& a, int64_t i, typename Acc<MODE>::type value, int64_t cnt, int64_t size)
{
  const bool counting = a.out_kind == O_COUNT_VALID || a.out_kind == O_COUNT_ALL;
  const bool ok       = counting ? size >= (int64_t)a.min_periods : cnt >= (int64_t)(a.min_periods > 1 ? a.min_periods : 1);
  if constexpr (MODE == M_COUNT) {
    static_cast<int32_t*>(a.out)[i] = ok ? (int32_t)(a.out_kind == O_COUNT_ALL ? size : cnt) : 0;
  } else if constexpr (MODE == M_FSUM) {
    const double v = ok ? value : 0.0;
    if (a.out_kind == O_F32) static_cast<float*>(a.out)[i] = (float)v;
    else if (a.out_kind == O_MEAN_F) static_cast<double*>(a.out)[i] = ok ? v / (double)cnt : 0.0;
    else static_cast<double*>(a.out)[i] = v;
  } else if constexpr (MODE == M_ISUM) {
    if (a.out_kind == O_MEAN_I) static_cast<double*>(a.out)[i] = ok ? (double)(int64_t)value / (double)cnt : 0.0;
    else if (a.out_kind == O_MEAN_U) static_cast<double*>(a.out)[i] = ok ? (double)value / (double)cnt : 0.0;
    else static_cast<uint64_t*>(a.out)[i] = ok ? value : 0ull;
  } else {
    const uint64_t key = value ^ a.inv;
    with_type(a.dtype, [&](auto tag) {
      using T = decltype(tag);
      T r     = T(0);
      if (ok) {
        if constexpr (std::is_floating_point<T>::value) {
          const uint64_t bits = key == ~0ull ? 0x7FF8000000000000ull : from_sortable<uint64_t, K_FTOTAL>(key, 0);
          double d;
          __builtin_memcpy(&d, &bits, 8);
          r = (T)d;
        } else if constexpr (std::is_signed<T>::value) {
          r = (T)(int64_t)(key ^ 0x8000000000000000ull);
        } else {
          r = (T)key;
        }
      }
      static_cast<T*>(a.out)[i] = r;
    });
  }
  return ok;
}

// The validity of the 64 consecutive rows a wave has just written goes out through store_wave_validity (gx_validity.hpp).  The null
// count is NOT kept there: one atomic per wave on one address cost 27 ms per 2^28 rows where many rows are null (xp_rolling, a bitmap
// at L = 2); it is counted from the finished bitmap instead (gx_bitmask_count: n / 8 bytes read).
__global__ void k_nulls_from_valid(int64_t* count, int64_t n) { *count = n - *count; }

// ---------------------------------------------------------------------------------------------- the row loop
template <int MODE, bool NULLABLE>
__global__ void __launch_bounds__(BT) k_roll_rows(Args a)
{
  using A         = typename Acc<MODE>::type;
  const int64_t i = (int64_t)blockIdx.x * BT + threadIdx.x;
  bool ok         = false;
  if (i < a.n) {
    int64_t gs, ge;
    group_of(a, i, gs, ge);
    const int64_t p = a.pcol ? (int64_t)a.pcol[i] : a.p, f = a.fcol ? (int64_t)a.fcol[i] : a.f;
    int64_t lo = i - p + 1, hi = i + f;
    lo = lo < gs ? gs : lo;
    hi = hi > ge - 1 ? ge - 1 : hi;
    const int64_t size = hi >= lo ? hi - lo + 1 : 0;
    A acc              = identity<MODE>();
    int64_t cnt        = NULLABLE ? 0 : size;
    if constexpr (MODE == M_COUNT) {
      if (NULLABLE)
        for (int64_t j = lo; j <= hi; ++j) cnt += bit_is_set(a.valid, a.bit0 + j) ? 1 : 0;
    } else {
      with_type(a.dtype, [&](auto tag) {
        using T     = decltype(tag);
        const T* in = static_cast<const T*>(a.in);
        for (int64_t j = lo; j <= hi; ++j) {
          if (NULLABLE && !bit_is_set(a.valid, a.bit0 + j)) continue;
          acc = combine<MODE>(acc, to_acc<MODE>(in[j], a.inv));
          if (NULLABLE) ++cnt;
        }
      });
    }
    ok = store_row<MODE>(a, i, acc, cnt, size);
  }
  store_wave_validity(a.out_valid, i & ~(int64_t)63, a.n, ok);
}

// ---------------------------------------------------------------------------------------------- the tile kernel
// the state of a segmented scan: f = a restart lies inside what was folded, v / c = the value and valid count since the last restart
template <typename A>
struct Seg {
  A v;
  uint32_t c;
  uint32_t f;
};
// a = the part folded first (earlier rows going forward, later rows going backward), b = the part that follows it
template <int MODE, bool REV, typename A>
__device__ __forceinline__ Seg<A> seg_join(Seg<A> a, Seg<A> b)
{
  if (b.f) return b;
  return Seg<A>{REV ? combine<MODE>(b.v, a.v) : combine<MODE>(a.v, b.v), a.c + b.c, a.f};
}
template <int MODE, bool REV>
struct SegOp {
  template <typename S>
  __device__ __forceinline__ S operator()(S a, S b) const
  {
    return seg_join<MODE, REV>(a, b);
  }
};

__device__ __forceinline__ int phys(int k, int items) { return k + k / items; }

template <int MODE, bool NULLABLE, int ITEMS>
__global__ void __launch_bounds__(BT) k_roll_tile(Args a, int left, int right)
{
  using A = typename Acc<MODE>::type;
  using S = Seg<A>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int WP = BT * (ITEMS + 1);             // padded region rows
  A* s_pre         = reinterpret_cast<A*>(smem);   // staged accumulators, then the forward scan
  A* s_suf         = s_pre + WP;                   // the backward scan
  S* s_wave        = reinterpret_cast<S*>(s_suf + WP);             // NWV forward + NWV backward wave aggregates
  uint16_t* s_cp   = reinterpret_cast<uint16_t*>(s_wave + 2 * NWV);  // valid counts of the two scans (NULLABLE)
  uint16_t* s_cs   = s_cp + (NULLABLE ? WP : 0);
  uint8_t* s_flag  = reinterpret_cast<uint8_t*>(s_cs + (NULLABLE ? WP : 0));

  const int tid         = threadIdx.x;
  const int64_t tile_lo = (int64_t)blockIdx.x * TILE;
  const int64_t r0      = tile_lo - left;  // row of region element 0
  const int w           = TILE + left + right;  // region rows: <= BT * ITEMS (host)
  const uint32_t L      = (uint32_t)(a.p + a.f);  // 1 <= L <= SPAN + 1 (host)
  constexpr bool SCANS  = !(MODE == M_COUNT && !NULLABLE);  // the counts of a column without a bitmap need no data at all

  if constexpr (SCANS) {
    // ---- A: the region, coalesced
    auto stage = [&](auto tag) {
      using T     = decltype(tag);
      const T* in = static_cast<const T*>(a.in);
      for (int k = tid; k < w; k += BT) {
        const int64_t row = r0 + k;
        uint8_t fl        = F_START | F_END;
        A acc             = identity<MODE>();
        if (row >= 0 && row < a.n) {
          int64_t gs, ge;
          group_of(a, row, gs, ge);
          fl = (row == gs ? F_START : 0) | (row == ge - 1 ? F_END : 0);
          if (!NULLABLE || bit_is_set(a.valid, a.bit0 + row)) {
            fl |= F_VALID;
            if constexpr (MODE != M_COUNT) acc = to_acc<MODE>(in[row], a.inv);
          }
        }
        const int q = phys(k, ITEMS);
        if constexpr (MODE != M_COUNT) s_pre[q] = acc;
        s_flag[q] = fl;
      }
    };
    if constexpr (MODE == M_COUNT) stage(uint8_t{});
    else with_type(a.dtype, stage);
    __syncthreads();

    // ---- B: this thread's ITEMS rows
    const int k0 = tid * ITEMS, q0 = k0 + tid;  // phys(k0 + j) = q0 + j
    A v[ITEMS];
    uint32_t headm = 0, tailm = 0, validm = 0;
    {
      uint32_t r        = 0;  // position of the row inside its segment
      const int64_t row = r0 + k0;
      if (k0 < w && row >= 0 && row < a.n) {
        int64_t gs, ge;
        group_of(a, row, gs, ge);
        r = (uint32_t)(row - gs) % L;
      }
#pragma unroll
      for (int j = 0; j < ITEMS; ++j) {
        const bool in = k0 + j < w;
        const uint8_t fl = in ? s_flag[q0 + j] : (uint8_t)(F_START | F_END);
        if constexpr (MODE != M_COUNT) v[j] = in ? s_pre[q0 + j] : identity<MODE>();
        else v[j] = 0;
        if (fl & F_START) r = 0;
        if (r == 0) headm |= 1u << j;
        if ((fl & F_END) || r == L - 1) tailm |= 1u << j;
        if (fl & F_VALID) validm |= 1u << j;
        r = r + 1 == L ? 0 : r + 1;
      }
    }
    const unsigned lane = lane_id(), wv = tid / GX_WAVE;
    const S none{identity<MODE>(), 0u, 0u};
    // forward: aggregate, exclusive carry over the threads before this one, then the rows again from the carry
    S fwd = none, bwd = none;
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) fwd = seg_join<MODE, false>(fwd, S{v[j], (validm >> j) & 1u, (headm >> j) & 1u});
#pragma unroll
    for (int j = ITEMS - 1; j >= 0; --j) bwd = seg_join<MODE, true>(bwd, S{v[j], (validm >> j) & 1u, (tailm >> j) & 1u});
    const S finc = wave_inclusive_scan(fwd, SegOp<MODE, false>());
    // backward over the lanes: the same scan on the mirrored wave
    const S binc = shfl(wave_inclusive_scan(shfl(bwd, (int)(GX_WAVE - 1 - lane)), SegOp<MODE, true>()), (int)(GX_WAVE - 1 - lane));
    if (lane == GX_WAVE - 1) s_wave[wv] = finc;
    if (lane == 0) s_wave[NWV + wv] = binc;
    __syncthreads();
    S fcar = none, bcar = none;
    for (unsigned k = 0; k < wv; ++k) fcar = seg_join<MODE, false>(fcar, s_wave[k]);
    for (unsigned k = NWV - 1; k > wv; --k) bcar = seg_join<MODE, true>(bcar, s_wave[NWV + k]);
    {
      S up = shfl_up(finc, 1);
      if (lane == 0) up = none;
      fcar = seg_join<MODE, false>(fcar, up);
      S dn = shfl(binc, (int)((lane + 1) & (GX_WAVE - 1)));
      if (lane == GX_WAVE - 1) dn = none;
      bcar = seg_join<MODE, true>(bcar, dn);
    }
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
      fcar = seg_join<MODE, false>(fcar, S{v[j], (validm >> j) & 1u, (headm >> j) & 1u});
      if (k0 + j < w) {
        if constexpr (MODE != M_COUNT) s_pre[q0 + j] = fcar.v;
        if constexpr (NULLABLE) s_cp[q0 + j] = (uint16_t)fcar.c;
      }
    }
#pragma unroll
    for (int j = ITEMS - 1; j >= 0; --j) {
      bcar = seg_join<MODE, true>(bcar, S{v[j], (validm >> j) & 1u, (tailm >> j) & 1u});
      if (k0 + j < w) {
        if constexpr (MODE != M_COUNT) s_suf[q0 + j] = bcar.v;
        if constexpr (NULLABLE) s_cs[q0 + j] = (uint16_t)bcar.c;
      }
    }
    __syncthreads();
  }

  // ---- C: the output rows; a wave writes 64 consecutive rows and their two validity words
#pragma unroll 1
  for (int r = 0; r < TILE / BT; ++r) {
    const int64_t i = tile_lo + r * BT + tid;
    bool ok         = false;
    if (i < a.n) {
      int64_t gs, ge;
      group_of(a, i, gs, ge);
      int64_t lo = i - a.p + 1, hi = i + a.f;
      lo = lo < gs ? gs : lo;
      hi = hi > ge - 1 ? ge - 1 : hi;
      const int64_t size = hi >= lo ? hi - lo + 1 : 0;
      A val              = identity<MODE>();
      int64_t cnt        = size;
      if (SCANS && size > 0) {
        const int ql = phys((int)(lo - r0), ITEMS), qh = phys((int)(hi - r0), ITEMS);  // 0 <= lo - r0 <= hi - r0 < w
        const uint32_t rlo = (uint32_t)(lo - gs) % L;
        if (rlo + (uint32_t)(size - 1) >= L) {  // two segments
          if constexpr (MODE != M_COUNT) val = combine<MODE>(s_suf[ql], s_pre[qh]);
          if constexpr (NULLABLE) cnt = (int64_t)s_cs[ql] + s_cp[qh];
        } else if (rlo == 0) {
          if constexpr (MODE != M_COUNT) val = s_pre[qh];
          if constexpr (NULLABLE) cnt = s_cp[qh];
        } else {
          if constexpr (MODE != M_COUNT) val = s_suf[ql];
          if constexpr (NULLABLE) cnt = s_cs[ql];
        }
      }
      ok = store_row<MODE>(a, i, val, cnt, size);
    }
    store_wave_validity(a.out_valid, i & ~(int64_t)63, a.n, ok);
  }
}

template <int MODE, bool NULLABLE, int ITEMS>
static size_t tile_lds_bytes()
{
  constexpr size_t WP = (size_t)BT * (ITEMS + 1);
  return WP * 16 + 2 * NWV * sizeof(Seg<typename Acc<MODE>::type>) + (NULLABLE ? WP * 4 : 0) + WP;
}

template <int MODE, bool NULLABLE, int ITEMS>
static int launch_tile_items(const Device& dev, const Args& a, int left, int right, hipStream_t s)
{
  const dim3 grid((unsigned)div_up(a.n, (int64_t)TILE));
  if (MODE == M_COUNT && !NULLABLE) {  // no region, no LDS
    hipLaunchKernelGGL((k_roll_tile<MODE, NULLABLE, ITEMS>), grid, dim3(BT), 0, s, a, left, right);
    return 0;
  }
  return launch_lds(dev, k_roll_tile<MODE, NULLABLE, ITEMS>, grid, dim3(BT), tile_lds_bytes<MODE, NULLABLE, ITEMS>(), s, a, left, right);
}
// region rows per thread: the smallest of 10 / 12 / 16 that holds TILE + halo (halo <= 512 / 1024 / 2048)
template <int MODE, bool NULLABLE>
static int launch_tile(const Device& dev, const Args& a, int left, int right, hipStream_t s)
{
  const int w = TILE + left + right;
  if ((MODE == M_COUNT && !NULLABLE) || w <= BT * 10) return launch_tile_items<MODE, NULLABLE, 10>(dev, a, left, right, s);
  if (w <= BT * 12) return launch_tile_items<MODE, NULLABLE, 12>(dev, a, left, right, s);
  return launch_tile_items<MODE, NULLABLE, 16>(dev, a, left, right, s);
}

template <int MODE, bool NULLABLE>
static int launch(bool tile, const Args& a, int left, int right, hipStream_t s)
{
  if (tile) {
    Device dev;
    GX_HIP_TRY(device(&dev));
    GX_HIP_TRY((launch_tile<MODE, NULLABLE>(dev, a, left, right, s)));
  } else {
    hipLaunchKernelGGL((k_roll_rows<MODE, NULLABLE>), dim3((unsigned)div_up(a.n, (int64_t)BT)), dim3(BT), 0, s, a);
  }
  GX_LAUNCH_CHECK();
  return 0;
}
template <int MODE>
static int launch_mode(bool tile, const Args& a, int left, int right, hipStream_t s)
{
  return a.valid ? launch<MODE, true>(tile, a, left, right, s) : launch<MODE, false>(tile, a, left, right, s);
}

static thread_local int g_kernel = 0;  // gx_rolling_set_kernel

}  // namespace roll
}  // namespace gx

extern "C" {

using namespace gx;
using namespace gx::roll;

int gx_rolling_tile_rows(void) { return TILE; }
int gx_rolling_max_span(void) { return SPAN; }
void gx_rolling_set_kernel(int which) { g_kernel = which >= 0 && which <= 2 ? which : 0; }

int gx_rolling_window(int dtype, const void* in, const uint32_t* in_valid, int64_t in_begin_bit, int64_t n, int64_t preceding,
                      int64_t following, const int32_t* preceding_col, const int32_t* following_col, const int32_t* labels,
                      const int32_t* offsets, int min_periods, int op, void* out, uint32_t* out_valid, int64_t* out_null_count_dev,
                      gx_stream_t stream)
{
  if (n < 0 || n > 0x7FFFFFFFll || min_periods < 0 || in_begin_bit < 0) return GX_EINVAL;
  if ((preceding_col == nullptr) != (following_col == nullptr)) return GX_EINVAL;
  if ((labels == nullptr) != (offsets == nullptr)) return GX_EINVAL;
  if (dtype < GX_INT8 || dtype > GX_BOOL8) return GX_EDTYPE;
  const bool is_float = dtype == GX_FLOAT32 || dtype == GX_FLOAT64;
  int mode;
  Args a{};
  switch (op) {
    case GX_OP_SUM:
      mode       = is_float ? M_FSUM : M_ISUM;
      a.out_kind = dtype == GX_FLOAT32 ? O_F32 : (dtype == GX_FLOAT64 ? O_F64 : O_BITS64);
      break;
    case GX_OP_MEAN:
      mode       = is_float ? M_FSUM : M_ISUM;
      a.out_kind = is_float ? O_MEAN_F : (dtype == GX_UINT64 ? O_MEAN_U : O_MEAN_I);
      break;
    case GX_OP_MIN:
    case GX_OP_MAX:
      mode       = M_MIN;
      a.out_kind = O_KEY;
      a.inv      = op == GX_OP_MAX ? ~0ull : 0ull;
      break;
    case GX_OP_COUNT_VALID:
    case GX_OP_COUNT_ALL:
      mode       = M_COUNT;
      a.out_kind = op == GX_OP_COUNT_ALL ? O_COUNT_ALL : O_COUNT_VALID;
      break;
    default: return GX_EDTYPE;
  }
  if (n > 0 && (!in || !out || !out_valid)) return GX_EINVAL;
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;

  constexpr int64_t FAR = 1ll << 31;  // a bound at or beyond +-2^31 rows from its row lies outside every column
  const int64_t p = preceding > FAR ? FAR : (preceding < -FAR ? -FAR : preceding);
  const int64_t f = following > FAR ? FAR : (following < -FAR ? -FAR : following);
  a.in    = in;
  a.valid = op == GX_OP_COUNT_ALL ? nullptr : in_valid;  // COUNT_ALL looks at no bitmap
  a.bit0  = in_begin_bit;
  a.n     = n;
  a.p     = p;
  a.f     = f;
  a.pcol  = preceding_col;
  a.fcol  = following_col;
  a.labels      = labels;
  a.offsets     = offsets;
  a.min_periods = min_periods;
  a.dtype       = dtype;
  a.out         = out;
  a.out_valid   = out_valid;

  const int64_t left = p > 1 ? p - 1 : 0, right = f > 0 ? f : 0;
  const bool applies = !preceding_col && p + f >= 1 && left + right <= SPAN;
  const bool tile    = applies && g_kernel != 2 && (g_kernel == 1 || p + f > DIRECT_MAX);
  int rc;
  switch (mode) {
    case M_ISUM: rc = launch_mode<M_ISUM>(tile, a, (int)left, (int)right, s); break;
    case M_FSUM: rc = launch_mode<M_FSUM>(tile, a, (int)left, (int)right, s); break;
    case M_MIN: rc = launch_mode<M_MIN>(tile, a, (int)left, (int)right, s); break;
    default: rc = launch_mode<M_COUNT>(tile, a, (int)left, (int)right, s); break;
  }
  if (rc != 0 || !out_null_count_dev) return rc;
  if (int rc2 = gx_bitmask_count(out_valid, 0, n, out_null_count_dev, stream)) return rc2;
  hipLaunchKernelGGL(k_nulls_from_valid, dim3(1), dim3(1), 0, s, out_null_count_dev, n);
  GX_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
