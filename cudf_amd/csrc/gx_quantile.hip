// gx_quantile.hip -- order statistics: cudf::quantile / quantiles, the MEDIAN and QUANTILE aggregations (the reference's
// cpp/src/quantiles/quantile.cu, quantiles.cu, reductions/quantile.cu, groupby/sort/group_quantiles.cu).
//
// INDEX AND INTERPOLATION RULES (stated here once; quantile_index / interpolate below are the only code that knows them).
// For `count` rows in order x[0 .. count) and a quantile q clamped to [0, 1]:
//   pos = q * (count - 1) in double;  lower = floor(pos), higher = ceil(pos), nearest = nearbyint(pos) (ties to even),
//   frac = pos - lower.
//   LOWER = x[lower], HIGHER = x[higher], NEAREST = x[nearest] (always one of the two);
//   LINEAR = (1 - frac) * double(a) + frac * double(b), MIDPOINT = double(a) / 2 + double(b) / 2 with a = x[lower], b = x[higher],
//   every product and sum rounded on its own (fp contraction off): the bits of NumPy float64 arithmetic on the host.
//   The inexact (exact = false) result is static_cast<T> of that double for LINEAR / MIDPOINT and the element itself, moved as
//   bits, for the other three.
// ORDER is the order of the sorts: the unsigned order of to_sortable (NaN greatest, -0.0 == +0.0), read through gx_rows.hpp; among
// equal sortable words the rows stand in input order, as in the stable gx_sort_keys.  Nulls are excluded.
//
// gx_quantile (an UNSORTED column) has two paths.
// SELECT, three streaming reads of the column instead of a sort:
//   k_range    min / max of the sortable words and the valid count (one set of atomics per workgroup);
//   k_hist     digit = (w - wmin) >> shift, shift chosen so that the digit is the top 11 bits of the span wmax - wmin (0 when the
//              span is below 2048); a workgroup counts in LDS (lds_count: a wave that hits one bin issues one atomic) and adds its
//              non-zero bins to one global table with device-scope atomics;
//   k_plan     one workgroup: prefix sums of the table, each q's lower / higher rank over the counted valid rows, the bin of each
//              rank, the wanted-bin bitmap, the exact candidate count c = rows in wanted bins, each rank's position among the
//              candidates.  With shift == 0 a bin IS a value and the plan is the answer (SELECT_DIRECT); so is wmin == wmax;
//   k_collect  appends the sortable words of the rows in wanted bins to a buffer of exactly c words.  A workgroup stages them in LDS
//              and reserves a run of the buffer with ONE global atomic per flush; every index, the LDS one and the global one, is
//              checked against its capacity: a violation sets a status bit (gx_quantile_status -> GX_EINTERNAL), never a fault.
//              BOUND: k_plan counts exactly the rows k_collect selects (same digit, same bitmap, same column), the cursor only
//              grows by flushed counts, so cursor <= c at every moment; the check is for bugs, not for data.
//   The buffer goes through gx_sort_keys as unsigned words of the column's width; k_finish reads the ranks and turns the words
//   back into elements.  A float word of the zero class or the NaN class stands for several bit patterns: the element is then
//   the k-th row of its class in input order (k = rank - rows below the class), found by k_tie_count / k_tie_pick -- two kernels
//   that exit at once unless k_finish flagged such a rank.
// SORT: valid rows compacted with the row-filter selectors when there is a bitmap, gx_sort_keys on all of them, ranks read.
// AUTO takes SORT below min_rows rows without looking at the column, and after the plan when c > max_share * n (one bin holds most
// rows: skew, or an outlier that stretches the span); gx_quantile_set_thresholds.
// The entry point reads the plan's head (valid count, c, shift) back ONCE per call and waits for the stream there.
//
// gx_quantile_lookup (order KNOWN: sorted data or an order map, optionally segmented) is the reference's own kernel shape: one
// thread per output.
#include <type_traits>

#include "gx_common.hpp"
#include "gx_rows.hpp"

namespace gx {
namespace quant {

constexpr int BT       = 256;
constexpr int ITEMS    = 8;
constexpr int TILE     = BT * ITEMS;  // rows of one workgroup trip: gx_quantile_tile_rows()
constexpr int NBINS    = 2048;
constexpr int MAXQ     = 64;
constexpr int MAXR     = 2 * MAXQ;   // ranks of one call: lower and higher of every q
constexpr int TIE_TILE = 8 * TILE;   // rows behind one pair of class counters
constexpr int FLUSH_AT = 2048;       // staged candidates at which a workgroup flushes
constexpr int STAGE    = FLUSH_AT + TILE;

enum { INTERP_LINEAR = 0, INTERP_LOWER = 1, INTERP_HIGHER = 2, INTERP_MIDPOINT = 3, INTERP_NEAREST = 4 };
enum { ST_COLLECT_GLOBAL = 1, ST_COLLECT_LDS = 2, ST_FINISH_POS = 4, ST_TIE_LOST = 8 };

struct QIndex {
  int64_t lower, higher, nearest;
  double frac;
};
__host__ __device__ inline QIndex quantile_index(int64_t count, double q)
{
  q                = q < 0.0 ? 0.0 : (q > 1.0 ? 1.0 : q);
  const double pos = q * (double)(count - 1);
  QIndex r;
  r.lower   = (int64_t)floor(pos);
  r.higher  = (int64_t)ceil(pos);
  r.nearest = (int64_t)nearbyint(pos);
  r.frac    = pos - (double)r.lower;
  return r;
}
// LINEAR / MIDPOINT of the two neighbours, LOWER / HIGHER / NEAREST as the neighbour's double
__host__ __device__ inline double interpolate(int interp, const QIndex& ix, double a, double b)
{
#pragma clang fp contract(off)
  switch (interp) {
    case INTERP_LINEAR: {
      const double pa = (1.0 - ix.frac) * a;
      const double pb = ix.frac * b;
      return pa + pb;
    }
    case INTERP_MIDPOINT: {
      const double ha = a / 2.0;
      const double hb = b / 2.0;
      return ha + hb;
    }
    case INTERP_LOWER: return a;
    case INTERP_HIGHER: return b;
    default: return ix.nearest == ix.lower ? a : b;
  }
}

// the digit rule: shift such that (w - wmin) >> shift keeps the top 11 bits of the span
__host__ __device__ inline int digit_shift(uint64_t span)
{
  if (span < (uint64_t)NBINS) return 0;
  return (64 - __builtin_clzll(span)) - 11;
}

template <typename U, int KIND>
__host__ __device__ inline double elem_to_double(U bits)
{
  if constexpr (KIND == K_FLOAT) {
    if constexpr (sizeof(U) == 4) {
      float f;
      __builtin_memcpy(&f, &bits, 4);
      return (double)f;
    } else {
      double d;
      __builtin_memcpy(&d, &bits, 8);
      return d;
    }
  } else if constexpr (KIND == K_SIGNED) {
    return (double)(std::make_signed_t<U>)bits;
  } else {
    return (double)bits;
  }
}
// static_cast<T>(d) as the bits of T
template <typename U, int KIND>
__device__ inline U double_to_elem(double d)
{
  if constexpr (KIND == K_FLOAT) {
    if constexpr (sizeof(U) == 4) {
      const float f = (float)d;
      U b;
      __builtin_memcpy(&b, &f, 4);
      return b;
    } else {
      U b;
      __builtin_memcpy(&b, &d, 8);
      return b;
    }
  } else if constexpr (KIND == K_SIGNED) {
    return (U)(std::make_signed_t<U>)d;
  } else {
    return (U)d;
  }
}
// sortable word -> element bits; *tie_class = 1 (zeros) / 2 (NaNs) when the word stands for several bit patterns
template <typename U, int KIND>
__device__ inline U word_to_elem(U w, uint32_t* tie_class)
{
  constexpr U SIGN = U(U(1) << (sizeof(U) * 8 - 1));
  *tie_class       = 0;
  if constexpr (KIND == K_FLOAT) {
    if (w == SIGN) *tie_class = 1;
    if (w == U(~U(0))) *tie_class = 2;
    return from_sortable<U, K_FTOTAL>(w, U(0));
  } else {
    return from_sortable<U, KIND>(w, U(0));
  }
}

struct QArgs {
  double q[MAXQ];
  int nq;
};

// the plan in device memory; the host reads the first PLAN_HOST_BYTES back
struct Head {
  unsigned long long wmin, wmax, nvalid, c, cursor;
  int32_t shift;
  uint32_t status, direct, tie_any;
  uint32_t wanted[NBINS / 32];
  unsigned long long pos[MAXR];    // position among the sorted candidates
  unsigned long long word[MAXR];   // SELECT_DIRECT: the sortable word itself
  unsigned long long elem[MAXR];   // the element's bits, zero-extended
  unsigned long long tie_k[MAXR];  // the rank's index inside its word's rows, in input order
  uint32_t tie_class[MAXR];
};
struct PlanHost {
  unsigned long long wmin, wmax, nvalid, c, cursor;
  int32_t shift;
  uint32_t status, direct, tie_any;
};

__global__ void __launch_bounds__(BT) k_init(Head* h, uint32_t* hist, unsigned long long nvalid0)
{
  const unsigned t = threadIdx.x;
  for (unsigned b = t; b < NBINS; b += BT) hist[b] = 0;
  if (t < NBINS / 32) h->wanted[t] = 0;
  if (t < MAXR) {
    h->pos[t] = h->word[t] = h->elem[t] = h->tie_k[t] = 0;
    h->tie_class[t]                                   = 0;
  }
  if (t == 0) {
    h->wmin   = ~0ull;
    h->wmax   = 0;
    h->nvalid = nvalid0;
    h->c = h->cursor = 0;
    h->shift         = 0;
    h->status = h->direct = h->tie_any = 0;
  }
}

// One workgroup trip: the TILE rows of `tile`, wave by wave in runs of 64 consecutive rows (the validity of a run comes from one
// bits_from64 at a wave-uniform address).  ok[s] / w[s]: validity and sortable word of this lane's row of step s; a null's bytes
// are not read.
template <typename U, int KIND>
__device__ __forceinline__ void load_tile(const void* data, const uint32_t* valid, int64_t bit0, int64_t n, int64_t tile, bool (&ok)[ITEMS],
                                          uint64_t (&w)[ITEMS])
{
  const unsigned lane = lane_id();
  const int64_t wave0 = tile * TILE + (int64_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / GX_WAVE)) * GX_WAVE;
#pragma unroll
  for (int s = 0; s < ITEMS; ++s) {
    const int64_t row0 = wave0 + (int64_t)s * BT;
    ok[s]              = false;
    w[s]               = 0;
    if (row0 < n) {
      const int64_t end = row0 + GX_WAVE < n ? row0 + GX_WAVE : n;
      const uint64_t vb = valid ? bits_from64(valid, bit0 + row0, bit0 + end) : low_mask64((int)(end - row0));
      ok[s]             = (vb >> lane) & 1ull;
      if (ok[s]) w[s] = rows::sortable_elem(data, (int)sizeof(U), KIND, 0, row0 + lane);
    }
  }
}

template <typename U, int KIND>
__global__ void __launch_bounds__(BT) k_range(const void* data, const uint32_t* valid, int64_t bit0, int64_t n, Head* h)
{
  __shared__ unsigned long long s_min[BT / GX_WAVE], s_max[BT / GX_WAVE], s_cnt[BT / GX_WAVE];
  unsigned long long mn = ~0ull, mx = 0, cnt = 0;
  const int64_t ntiles = div_up(n, TILE);
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    bool ok[ITEMS];
    uint64_t w[ITEMS];
    load_tile<U, KIND>(data, valid, bit0, n, tile, ok, w);
#pragma unroll
    for (int s = 0; s < ITEMS; ++s) {
      if (ok[s]) {
        mn = w[s] < mn ? w[s] : mn;
        mx = w[s] > mx ? w[s] : mx;
        ++cnt;
      }
    }
  }
  mn  = wave_reduce(mn, MinOp());
  mx  = wave_reduce(mx, MaxOp());
  cnt = wave_reduce(cnt, SumOp());
  if (lane_id() == 0) {
    s_min[threadIdx.x / GX_WAVE] = mn;
    s_max[threadIdx.x / GX_WAVE] = mx;
    s_cnt[threadIdx.x / GX_WAVE] = cnt;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < BT / GX_WAVE; ++k) {
      mn = s_min[k] < mn ? s_min[k] : mn;
      mx = s_max[k] > mx ? s_max[k] : mx;
      cnt += s_cnt[k];
    }
    if (cnt) {  // device-scope atomics: the workgroups sit on eight XCDs
      atomicMin(&h->wmin, mn);
      atomicMax(&h->wmax, mx);
      atomicAdd(&h->nvalid, cnt);
    }
  }
}

template <typename U, int KIND>
__global__ void __launch_bounds__(BT) k_hist(const void* data, const uint32_t* valid, int64_t bit0, int64_t n, const Head* h, uint32_t* hist)
{
  __shared__ uint32_t s_hist[NBINS];
  const unsigned long long wmin = h->wmin, wmax = h->wmax;
  if (h->nvalid == 0 || wmin == wmax) return;  // nothing to count: the plan answers
  const int shift = digit_shift(wmax - wmin);
  for (unsigned b = threadIdx.x; b < NBINS; b += BT) s_hist[b] = 0;
  __syncthreads();
  const int64_t ntiles = div_up(n, TILE);
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    bool ok[ITEMS];
    uint64_t w[ITEMS];
    load_tile<U, KIND>(data, valid, bit0, n, tile, ok, w);
#pragma unroll
    for (int s = 0; s < ITEMS; ++s) {
      const uint32_t d = ok[s] ? (uint32_t)((w[s] - wmin) >> shift) : 0u;
      lds_count(s_hist, d < NBINS ? d : NBINS - 1, ok[s]);
    }
  }
  __syncthreads();
  for (unsigned b = threadIdx.x; b < NBINS; b += BT) {
    const uint32_t v = s_hist[b];
    if (v) atomicAdd(&hist[b], v);
  }
}

// One workgroup.  pre[b] = valid rows in bins below b; a rank r lies in the last bin with pre[b] <= r.
__global__ void __launch_bounds__(BT) k_plan(Head* h, const uint32_t* hist, QArgs qa)
{
  __shared__ uint32_t s_cnt[NBINS], s_pre[NBINS], s_wanted[NBINS / 32], s_scan[BT / GX_WAVE + 1];
  __shared__ uint32_t s_bin[MAXR], s_off[MAXR];
  const unsigned t              = threadIdx.x;
  const unsigned long long nv   = h->nvalid;
  const unsigned long long wmin = h->wmin, wmax = h->wmax;
  const int nr                  = 2 * qa.nq;
  if (nv == 0) return;
  unsigned long long rank = 0;
  if ((int)t < nr) {
    const QIndex ix = quantile_index((int64_t)nv, qa.q[t >> 1]);
    rank            = (unsigned long long)((t & 1) ? ix.higher : ix.lower);
  }
  if (wmin == wmax) {  // every valid row is one word
    if ((int)t < nr) {
      h->word[t]  = wmin;
      h->tie_k[t] = rank;
    }
    if (t == 0) h->direct = 1;
    return;
  }
  const int shift = digit_shift(wmax - wmin);
  for (unsigned b = t; b < NBINS; b += BT) s_cnt[b] = hist[b];
  if (t < NBINS / 32) s_wanted[t] = 0;
  __syncthreads();
  constexpr int PER = NBINS / BT;
  {
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) sum += s_cnt[t * PER + k];
    uint32_t run = block_exclusive_scan<BT>(sum, 0u, SumOp(), s_scan, (uint32_t*)nullptr);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      s_pre[t * PER + k] = run;
      run += s_cnt[t * PER + k];
    }
  }
  __syncthreads();
  if ((int)t < nr) {
    int lo = 0, hi = NBINS;  // last b with s_pre[b] <= rank (s_pre[0] = 0 <= rank)
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if ((unsigned long long)s_pre[mid] <= rank) lo = mid;
      else hi = mid;
    }
    s_bin[t] = (uint32_t)lo;
    s_off[t] = (uint32_t)(rank - s_pre[lo]);
    atomicOr(&s_wanted[lo >> 5], 1u << (lo & 31));
  }
  __syncthreads();
  uint32_t total = 0;
  {
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const unsigned b = t * PER + k;
      sum += ((s_wanted[b >> 5] >> (b & 31)) & 1u) ? s_cnt[b] : 0u;
    }
    uint32_t run = block_exclusive_scan<BT>(sum, 0u, SumOp(), s_scan, &total);
#pragma unroll
    for (int k = 0; k < PER; ++k) {  // s_pre becomes the prefix over WANTED bins
      const unsigned b = t * PER + k;
      s_pre[b]         = run;
      run += ((s_wanted[b >> 5] >> (b & 31)) & 1u) ? s_cnt[b] : 0u;
    }
  }
  __syncthreads();
  if ((int)t < nr) {
    h->pos[t]   = (unsigned long long)s_pre[s_bin[t]] + s_off[t];
    h->word[t]  = wmin + s_bin[t];  // meaningful with shift == 0 only
    h->tie_k[t] = s_off[t];         // with shift == 0 a bin is one word
  }
  if (t < NBINS / 32) h->wanted[t] = s_wanted[t];
  if (t == 0) {
    h->shift  = shift;
    h->direct = shift == 0 ? 1u : 0u;
    h->c      = shift == 0 ? 0ull : (unsigned long long)total;
  }
}

template <typename U, int KIND>
__global__ void __launch_bounds__(BT) k_collect(const void* data, const uint32_t* valid, int64_t bit0, int64_t n, Head* h, U* cand)
{
  __shared__ U s_buf[STAGE];
  __shared__ uint32_t s_wanted[NBINS / 32];
  __shared__ uint32_t s_n;
  __shared__ unsigned long long s_base;
  const unsigned long long wmin = h->wmin, c = h->c;
  const int shift               = h->shift;
  if (threadIdx.x < NBINS / 32) s_wanted[threadIdx.x] = h->wanted[threadIdx.x];
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  // flush the staged words: ONE global atomic reserves the run, every store is checked against c
  auto flush = [&]() {
    const uint32_t cnt = s_n;  // uniform: read behind a barrier
    if (cnt == 0) return;
    if (threadIdx.x == 0) s_base = atomicAdd(&h->cursor, (unsigned long long)cnt);
    __syncthreads();
    const unsigned long long base = s_base;
    for (uint32_t i = threadIdx.x; i < cnt; i += BT) {
      if (base + i < c) cand[base + i] = s_buf[i];
      else atomicOr(&h->status, (uint32_t)ST_COLLECT_GLOBAL);
    }
    __syncthreads();
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
  };
  const int64_t ntiles = div_up(n, TILE);
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    bool ok[ITEMS];
    uint64_t w[ITEMS];
    load_tile<U, KIND>(data, valid, bit0, n, tile, ok, w);
#pragma unroll
    for (int s = 0; s < ITEMS; ++s) {
      uint32_t d = ok[s] ? (uint32_t)((w[s] - wmin) >> shift) : 0u;
      d          = d < NBINS ? d : NBINS - 1;
      const bool want   = ok[s] && ((s_wanted[d >> 5] >> (d & 31)) & 1u);
      const uint64_t wb = ballot(want);
      if (wb) {  // one LDS atomic per wave reserves its rows of the stage
        uint32_t base = 0;
        if (lane_id() == (unsigned)__builtin_ctzll(wb)) base = atomicAdd(&s_n, (uint32_t)__builtin_popcountll(wb));
        base               = shfl(base, __builtin_ctzll(wb));
        const uint32_t idx = base + (uint32_t)__builtin_popcountll(wb & lanemask_lt());
        if (want) {
          if (idx < (uint32_t)STAGE) s_buf[idx] = (U)w[s];
          else atomicOr(&h->status, (uint32_t)ST_COLLECT_LDS);
        }
      }
    }
    __syncthreads();
    if (s_n >= (uint32_t)FLUSH_AT) flush();  // s_n < FLUSH_AT in front of every trip, a trip adds at most TILE
    else __syncthreads();                    // (the reads of s_n above are done before the next trip's atomics)
  }
  __syncthreads();
  if (s_n > (uint32_t)STAGE) {  // only behind an LDS violation: keep the copy inside the stage
    __syncthreads();
    if (threadIdx.x == 0) s_n = STAGE;
    __syncthreads();
  }
  flush();
}

// SRC 0: the plan's words (SELECT_DIRECT); 1: the sorted candidate words at the plan's positions; 2: a sorted copy of the valid rows
// in the column's own type, read at the ranks.  One thread per rank.
template <typename U, int KIND, int SRC>
__global__ void __launch_bounds__(MAXR) k_finish(Head* h, const U* sorted, QArgs qa)
{
  const int t                 = (int)threadIdx.x;
  const unsigned long long nv = h->nvalid;
  if (t >= 2 * qa.nq || nv == 0) return;
  if constexpr (SRC == 2) {
    const QIndex ix = quantile_index((int64_t)nv, qa.q[t >> 1]);
    h->elem[t]      = (unsigned long long)sorted[(t & 1) ? ix.higher : ix.lower];
    return;
  } else {
    U w;
    unsigned long long k;
    if constexpr (SRC == 0) {
      w = (U)h->word[t];
      k = h->tie_k[t];
    } else {
      const unsigned long long c = h->c, p = h->pos[t];
      if (p >= c) {
        atomicOr(&h->status, (uint32_t)ST_FINISH_POS);
        return;
      }
      w = sorted[p];
      unsigned long long lo = 0, hi = p;  // first position that holds w
      while (lo < hi) {
        const unsigned long long mid = (lo + hi) >> 1;
        if (sorted[mid] < w) lo = mid + 1;
        else hi = mid;
      }
      k = p - lo;
    }
    uint32_t cls;
    h->elem[t] = (unsigned long long)word_to_elem<U, KIND>(w, &cls);
    if (cls) {
      h->tie_class[t] = cls;
      h->tie_k[t]     = k;
      h->tie_any      = 1;
    }
  }
}

// float columns: rows of the zero class / the NaN class per TIE_TILE rows
template <typename U>
__global__ void __launch_bounds__(BT) k_tie_count(const void* data, const uint32_t* valid, int64_t bit0, int64_t n, const Head* h,
                                                  uint32_t* tiecnt)
{
  constexpr U SIGN = U(U(1) << (sizeof(U) * 8 - 1));
  __shared__ uint32_t s_z, s_n;
  if (h->tie_any == 0) return;
  const int64_t nties = div_up(n, TIE_TILE);
  for (int64_t tt = blockIdx.x; tt < nties; tt += gridDim.x) {
    if (threadIdx.x == 0) s_z = s_n = 0;
    __syncthreads();
    uint32_t z = 0, nn = 0;
    for (int64_t tile = tt * (TIE_TILE / TILE); tile < (tt + 1) * (TIE_TILE / TILE) && tile * TILE < n; ++tile) {
      bool ok[ITEMS];
      uint64_t w[ITEMS];
      load_tile<U, K_FLOAT>(data, valid, bit0, n, tile, ok, w);
#pragma unroll
      for (int s = 0; s < ITEMS; ++s) {
        z += (ok[s] && (U)w[s] == SIGN) ? 1u : 0u;
        nn += (ok[s] && (U)w[s] == U(~U(0))) ? 1u : 0u;
      }
    }
    z  = wave_reduce(z, SumOp());
    nn = wave_reduce(nn, SumOp());
    if (lane_id() == 0) {
      if (z) atomicAdd(&s_z, z);
      if (nn) atomicAdd(&s_n, nn);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      tiecnt[2 * tt]     = s_z;
      tiecnt[2 * tt + 1] = s_n;
    }
    __syncthreads();
  }
}
// workgroup j settles rank j: the tile that holds the tie_k-th row of the class, then that row, both by prefix sums in row order
template <typename U>
__global__ void __launch_bounds__(BT) k_tie_pick(const void* data, const uint32_t* valid, int64_t bit0, int64_t n, Head* h,
                                                 const uint32_t* tiecnt)
{
  constexpr U SIGN = U(U(1) << (sizeof(U) * 8 - 1));
  __shared__ unsigned long long s_scan[BT / GX_WAVE + 1];
  __shared__ long long s_tile;
  __shared__ unsigned long long s_rem;
  const int j = (int)blockIdx.x;
  if (h->tie_any == 0 || h->tie_class[j] == 0) return;
  const int cls       = (int)h->tie_class[j] - 1;
  const U want        = cls == 0 ? SIGN : U(~U(0));
  const int64_t nties = div_up(n, TIE_TILE);
  if (threadIdx.x == 0) s_tile = -1;
  __syncthreads();
  unsigned long long rem = h->tie_k[j];
  for (int64_t base = 0; base < nties; base += BT) {
    const int64_t tt           = base + threadIdx.x;
    const unsigned long long v = tt < nties ? tiecnt[2 * tt + cls] : 0ull;
    unsigned long long total   = 0;
    const unsigned long long e = block_exclusive_scan<BT>(v, 0ull, SumOp(), s_scan, &total);
    if (rem < total) {  // uniform
      if (e <= rem && rem < e + v) {
        s_tile = tt;
        s_rem  = rem - e;
      }
      break;
    }
    rem -= total;
  }
  __syncthreads();
  if (s_tile < 0) {
    if (threadIdx.x == 0) atomicOr(&h->status, (uint32_t)ST_TIE_LOST);
    return;
  }
  const int64_t row_begin = s_tile * TIE_TILE;
  rem                     = s_rem;
  __syncthreads();
  for (int64_t r0 = row_begin; r0 < row_begin + TIE_TILE && r0 < n; r0 += BT) {
    const int64_t row = r0 + threadIdx.x;
    bool hit          = false;
    if (row < n && row_valid(valid, bit0 + row)) hit = (U)rows::sortable_elem(data, (int)sizeof(U), K_FLOAT, 0, row) == want;
    unsigned long long total   = 0;
    const unsigned long long e = block_exclusive_scan<BT>(hit ? 1ull : 0ull, 0ull, SumOp(), s_scan, &total);
    if (rem < total) {
      if (hit && e == rem) h->elem[j] = rows::load_bits(data, (int)sizeof(U), row);
      return;
    }
    rem -= total;
  }
  if (threadIdx.x == 0) atomicOr(&h->status, (uint32_t)ST_TIE_LOST);
}

template <typename U, int KIND>
__global__ void __launch_bounds__(MAXQ) k_interp(const Head* h, QArgs qa, int interp, double* out_f64, U* out_elems, int64_t* nvalid_dev)
{
  const int t                 = (int)threadIdx.x;
  const unsigned long long nv = h->nvalid;
  if (t == 0) *nvalid_dev = (int64_t)nv;
  if (t >= qa.nq) return;
  const U a = nv ? (U)h->elem[2 * t] : U(0), b = nv ? (U)h->elem[2 * t + 1] : U(0);
  if (out_elems) {
    out_elems[2 * t]     = a;
    out_elems[2 * t + 1] = b;
  }
  const QIndex ix = quantile_index(nv ? (int64_t)nv : 1, qa.q[t]);
  out_f64[t]      = nv ? interpolate(interp, ix, elem_to_double<U, KIND>(a), elem_to_double<U, KIND>(b)) : 0.0;
}

// ---------------------------------------------------------------- lookup: one thread per output, group-major
template <typename U, int KIND>
__global__ void __launch_bounds__(BT) k_lookup(const void* data, const uint32_t* valid, int64_t bit0, const int32_t* order, int64_t nseg,
                                               const int32_t* offsets, const int32_t* counts, QArgs qa, int interp, int exact, void* out,
                                               uint32_t* out_valid, unsigned long long* null_count)
{
  __shared__ unsigned int s_nulls;
  tally_begin(&s_nulls);
  const int64_t total     = nseg * qa.nq;
  const unsigned lane     = lane_id();
  unsigned int wave_nulls = 0;
  for (int64_t first = (int64_t)blockIdx.x * BT + (threadIdx.x / GX_WAVE) * GX_WAVE; first < total; first += (int64_t)gridDim.x * BT) {
    const int64_t o = first + lane;
    bool ok         = false;
    if (o < total) {
      const int64_t seg = o / qa.nq;
      const int j       = (int)(o - seg * qa.nq);
      const int64_t beg = offsets[seg];
      const int64_t cnt = counts ? (int64_t)counts[seg] : (int64_t)offsets[seg + 1] - beg;
      U res_bits        = 0;
      double res        = 0.0;
      if (cnt > 0) {
        const QIndex ix    = quantile_index(cnt, qa.q[j]);
        const bool need_a  = interp == INTERP_LINEAR || interp == INTERP_MIDPOINT || interp == INTERP_LOWER ||
                            (interp == INTERP_NEAREST && ix.nearest == ix.lower);
        const bool need_b  = interp == INTERP_LINEAR || interp == INTERP_MIDPOINT || interp == INTERP_HIGHER ||
                            (interp == INTERP_NEAREST && ix.nearest != ix.lower);
        const int64_t ra   = order ? (int64_t)order[beg + ix.lower] : beg + ix.lower;
        const int64_t rb   = order ? (int64_t)order[beg + ix.higher] : beg + ix.higher;
        const bool va      = !need_a || row_valid(valid, bit0 + ra);
        const bool vb      = !need_b || row_valid(valid, bit0 + rb);
        ok                 = va && vb;
        if (ok) {
          const U a  = need_a ? (U)rows::load_bits(data, (int)sizeof(U), ra) : U(0);
          const U b  = need_b ? (U)rows::load_bits(data, (int)sizeof(U), rb) : U(0);
          res        = interpolate(interp, ix, elem_to_double<U, KIND>(a), elem_to_double<U, KIND>(b));
          res_bits   = (interp == INTERP_LINEAR || interp == INTERP_MIDPOINT) ? double_to_elem<U, KIND>(res) : (need_a ? a : b);
        }
      }
      if (exact) static_cast<double*>(out)[o] = res;
      else static_cast<U*>(out)[o] = res_bits;
    }
    const uint64_t vbits = out_valid ? store_wave_validity(out_valid, first, total, ok) : ballot(ok);
    const int64_t live   = total - first < GX_WAVE ? total - first : GX_WAVE;
    wave_nulls += (unsigned int)__builtin_popcountll(~vbits & low_mask64((int)live));
  }
  tally_end(&s_nulls, wave_nulls, null_count);
}

// ---------------------------------------------------------------- host
inline int unsigned_dtype(int width) { return width == 1 ? GX_UINT8 : width == 2 ? GX_UINT16 : width == 4 ? GX_UINT32 : GX_UINT64; }

inline bool fill_q(QArgs& qa, const double* q_host, int nq)
{
  qa    = QArgs{};
  qa.nq = nq;
  for (int j = 0; j < nq; ++j) {
    if (q_host[j] != q_host[j]) return false;
    qa.q[j] = q_host[j] < 0.0 ? 0.0 : (q_host[j] > 1.0 ? 1.0 : q_host[j]);
  }
  return true;
}

struct Scratch {
  Head* head;
  uint32_t* hist;
  void* buf_a;  // candidates, or the compacted valid rows
  void* buf_b;  // their sorted copy
  void* sort_tmp;
  size_t sort_bytes;
  void* sel_tmp;
  size_t sel_bytes;
  uint32_t* tiecnt;
  size_t bytes;
};
inline int carve(void* tmp, int dtype, int width, int kind, int64_t n, bool has_bitmap, Scratch& sc)
{
  Carver cv(tmp);
  sc.head = cv.take<Head>(1);
  sc.hist = cv.take<uint32_t>(NBINS);
  const size_t rows = (size_t)(n > 0 ? n : 1);
  sc.buf_a = cv.take<char>(rows * width);
  sc.buf_b = cv.take<char>(rows * width);
  size_t own = 0, words = 0;  // the larger of the two sorts a call may run, both with their output given
  int rc = gx_sort_keys(dtype, nullptr, reinterpret_cast<void*>(256), n, 0, nullptr, &own, nullptr);
  if (rc) return rc;
  rc = gx_sort_keys(unsigned_dtype(width), nullptr, reinterpret_cast<void*>(256), n, 0, nullptr, &words, nullptr);
  if (rc) return rc;
  sc.sort_bytes = own > words ? own : words;
  sc.sort_tmp   = cv.take<char>(sc.sort_bytes);
  sc.sel_bytes  = has_bitmap ? gx_compact_plan_bytes(n) : 0;
  sc.sel_tmp    = cv.take<char>(sc.sel_bytes);
  sc.tiecnt     = cv.take<uint32_t>(kind == K_FLOAT ? 2 * (size_t)div_up(rows, TIE_TILE) : 0);
  sc.bytes      = cv.total();
  return 0;
}

static thread_local int64_t g_min_rows  = 1 << 20;
static thread_local double g_max_share  = 0.5;

}  // namespace quant
}  // namespace gx

extern "C" {

using namespace gx;
using namespace gx::quant;

int gx_quantile_tile_rows(void) { return TILE; }

void gx_quantile_set_thresholds(int64_t min_rows, double max_share)
{
  g_min_rows  = min_rows < 0 ? (1 << 20) : min_rows;
  g_max_share = (max_share >= 0.0 && max_share <= 1.0) ? max_share : 0.5;
}
void gx_quantile_get_thresholds(int64_t* min_rows, double* max_share)
{
  if (min_rows) *min_rows = g_min_rows;
  if (max_share) *max_share = g_max_share;
}

int gx_quantile_index(int64_t count, double q, int64_t* lower, int64_t* higher, int64_t* nearest, double* frac)
{
  if (count < 1 || q != q || !lower || !higher || !nearest || !frac) return GX_EINVAL;
  const QIndex ix = quantile_index(count, q);
  *lower          = ix.lower;
  *higher         = ix.higher;
  *nearest        = ix.nearest;
  *frac           = ix.frac;
  return 0;
}

int gx_quantile_status(const void* tmp, int* status_host, gx_stream_t stream)
{
  if (!tmp || !status_host) return GX_EINVAL;
  PlanHost ph;
  GX_HIP_TRY(hipMemcpyAsync(&ph, tmp, sizeof(PlanHost), hipMemcpyDeviceToHost, (hipStream_t)stream));
  GX_HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  *status_host = (int)ph.status;
  return ph.status ? GX_EINTERNAL : 0;
}

int gx_quantile(int dtype, const void* data, const uint32_t* valid, int64_t valid_begin_bit, int64_t n, const double* q_host, int nq,
                int interp, int mode, double* out_f64_dev, void* out_elems_dev, int64_t* nvalid_dev, int* path_host, void* tmp,
                size_t* tmp_bytes, gx_stream_t stream)
{
  int kind = 0, width = 0;
  if (dtype == GX_BOOL8 || rows::key_kind_width(dtype, &kind, &width)) return GX_EDTYPE;  // GX_BOOL8 too: a quantile of booleans is not defined
  if (n < 0 || n >= (int64_t(1) << 31) || !tmp_bytes || !q_host || nq < 1 || nq > MAXQ || valid_begin_bit < 0) return GX_EINVAL;
  if (interp < INTERP_LINEAR || interp > INTERP_NEAREST || mode < GX_QUANTILE_AUTO || mode > GX_QUANTILE_FORCE_SORT) return GX_EINVAL;
  QArgs qa;
  if (!fill_q(qa, q_host, nq)) return GX_EINVAL;
  Scratch sc;
  {
    const int rc = carve(tmp, dtype, width, kind, n, valid != nullptr, sc);
    if (rc) return rc;
  }
  if (tmp && (!out_f64_dev || !nvalid_dev || (n > 0 && !data))) return GX_EINVAL;
  if (int rc; !scratch_ready(tmp, sc.bytes, tmp_bytes, &rc)) return rc;
  hipStream_t s = (hipStream_t)stream;
  Device dev;
  GX_HIP_TRY(device(&dev));
  const unsigned grid = capped_grid(n, TILE, (int64_t)dev.cus * 8);

  return with_dtype(dtype, [&](auto t) -> int {
    using U            = typename decltype(t)::word_type;
    constexpr int KIND = decltype(t)::kind;
    auto interp_out    = [&](int path) -> int {
      hipLaunchKernelGGL((k_interp<U, KIND>), dim3(1), dim3(MAXQ), 0, s, sc.head, qa, interp, out_f64_dev, static_cast<U*>(out_elems_dev),
                         nvalid_dev);
      GX_LAUNCH_CHECK();
      if (path_host) *path_host = path;
      return 0;
    };
    auto settle_ties = [&]() -> int {
      if constexpr (KIND == K_FLOAT) {
        hipLaunchKernelGGL((k_tie_count<U>), dim3(capped_grid(n, TIE_TILE, (int64_t)dev.cus * 8)), dim3(BT), 0, s, data, valid,
                           valid_begin_bit, n, sc.head, sc.tiecnt);
        GX_LAUNCH_CHECK();
        hipLaunchKernelGGL((k_tie_pick<U>), dim3(2 * nq), dim3(BT), 0, s, data, valid, valid_begin_bit, n, sc.head, sc.tiecnt);
        GX_LAUNCH_CHECK();
      }
      return 0;
    };
    const bool try_select = n > 0 && (mode == GX_QUANTILE_FORCE_SELECT || (mode == GX_QUANTILE_AUTO && n >= g_min_rows));
    PlanHost ph{};
    bool nvalid_known = false;
    if (try_select) {
      hipLaunchKernelGGL(k_init, dim3(1), dim3(BT), 0, s, sc.head, sc.hist, 0ull);
      hipLaunchKernelGGL((k_range<U, KIND>), dim3(grid), dim3(BT), 0, s, data, valid, valid_begin_bit, n, sc.head);
      hipLaunchKernelGGL((k_hist<U, KIND>), dim3(grid), dim3(BT), 0, s, data, valid, valid_begin_bit, n, sc.head, sc.hist);
      hipLaunchKernelGGL(k_plan, dim3(1), dim3(BT), 0, s, sc.head, sc.hist, qa);
      GX_LAUNCH_CHECK();
      GX_HIP_TRY(hipMemcpyAsync(&ph, sc.head, sizeof(PlanHost), hipMemcpyDeviceToHost, s));  // the one read-back of the call
      GX_HIP_TRY(hipStreamSynchronize(s));
      nvalid_known = true;
      if (ph.nvalid == 0) return interp_out(GX_QUANTILE_PATH_SELECT_DIRECT);
      if (ph.direct) {
        hipLaunchKernelGGL((k_finish<U, KIND, 0>), dim3(1), dim3(MAXR), 0, s, sc.head, (const U*)nullptr, qa);
        GX_LAUNCH_CHECK();
        if (int rc = settle_ties()) return rc;
        return interp_out(GX_QUANTILE_PATH_SELECT_DIRECT);
      }
      if (mode == GX_QUANTILE_FORCE_SELECT || (double)ph.c <= g_max_share * (double)n) {
        if (ph.c > (unsigned long long)n) return GX_EINTERNAL;
        hipLaunchKernelGGL((k_collect<U, KIND>), dim3(grid), dim3(BT), 0, s, data, valid, valid_begin_bit, n, sc.head,
                           static_cast<U*>(sc.buf_a));
        GX_LAUNCH_CHECK();
        size_t sb = sc.sort_bytes;
        if (int rc = gx_sort_keys(unsigned_dtype(width), sc.buf_a, sc.buf_b, (int64_t)ph.c, 0, sc.sort_tmp, &sb, stream)) return rc;
        hipLaunchKernelGGL((k_finish<U, KIND, 1>), dim3(1), dim3(MAXR), 0, s, sc.head, static_cast<const U*>(sc.buf_b), qa);
        GX_LAUNCH_CHECK();
        if (int rc = settle_ties()) return rc;
        return interp_out(GX_QUANTILE_PATH_SELECT);
      }
    }
    // ---- SORT
    hipLaunchKernelGGL(k_init, dim3(1), dim3(BT), 0, s, sc.head, sc.hist, (unsigned long long)(valid ? 0 : n));
    GX_LAUNCH_CHECK();
    const void* src = data;
    int64_t m       = n;
    if (valid && n > 0) {
      const uint32_t* vp[1] = {valid};
      const int64_t vb[1]   = {valid_begin_bit};
      size_t selb           = sc.sel_bytes;
      if (int rc = gx_select_valid_count(1, vp, vb, n, 1, reinterpret_cast<int64_t*>(&sc.head->nvalid), sc.sel_tmp, &selb, stream)) return rc;
      if (!nvalid_known) {
        GX_HIP_TRY(hipMemcpyAsync(&ph.nvalid, &sc.head->nvalid, sizeof(ph.nvalid), hipMemcpyDeviceToHost, s));  // the one read-back
        GX_HIP_TRY(hipStreamSynchronize(s));
      }
      m = (int64_t)ph.nvalid;
      if (m < 0 || m > n) return GX_EINTERNAL;
      if (m > 0) {
        if (int rc = gx_compact_column(width, data, nullptr, 0, n, sc.sel_tmp, sc.buf_a, nullptr, nullptr, stream)) return rc;
      }
      src = sc.buf_a;
    }
    if (m > 0) {
      size_t sb = sc.sort_bytes;
      if (int rc = gx_sort_keys(dtype, src, sc.buf_b, m, 0, sc.sort_tmp, &sb, stream)) return rc;
      hipLaunchKernelGGL((k_finish<U, KIND, 2>), dim3(1), dim3(MAXR), 0, s, sc.head, static_cast<const U*>(sc.buf_b), qa);
      GX_LAUNCH_CHECK();
    }
    return interp_out(GX_QUANTILE_PATH_SORT);
  });
}

int gx_quantile_lookup(int dtype, const void* data, const uint32_t* valid, int64_t begin_bit, const int32_t* order, int64_t nseg,
                       const int32_t* offsets_dev, const int32_t* seg_counts_dev, const double* q_host, int nq, int interp, int exact,
                       void* out, uint32_t* out_valid, int64_t* out_null_count_dev, gx_stream_t stream)
{
  int kind = 0, width = 0;
  if (dtype == GX_BOOL8 || rows::key_kind_width(dtype, &kind, &width)) return GX_EDTYPE;  // GX_BOOL8 too: a quantile of booleans is not defined
  if (nseg < 0 || !q_host || nq < 1 || nq > MAXQ || begin_bit < 0 || interp < INTERP_LINEAR || interp > INTERP_NEAREST) return GX_EINVAL;
  if (nseg * nq >= (int64_t(1) << 31)) return GX_EINVAL;
  QArgs qa;
  if (!fill_q(qa, q_host, nq)) return GX_EINVAL;
  if (nseg > 0 && (!offsets_dev || !out)) return GX_EINVAL;  // (data may be NULL: every segment may be empty)
  hipStream_t s = (hipStream_t)stream;
  if (out_null_count_dev) GX_HIP_TRY(hipMemsetAsync(out_null_count_dev, 0, sizeof(int64_t), s));
  if (nseg == 0) return 0;
  return with_dtype(dtype, [&](auto t) -> int {
    using U            = typename decltype(t)::word_type;
    constexpr int KIND = decltype(t)::kind;
    hipLaunchKernelGGL((k_lookup<U, KIND>), dim3(capped_grid(nseg * nq, BT, 4096)), dim3(BT), 0, s, data, valid, begin_bit, order, nseg,
                       offsets_dev, seg_counts_dev, qa, interp, exact ? 1 : 0, out, out_valid,
                       reinterpret_cast<unsigned long long*>(out_null_count_dev));
    GX_LAUNCH_CHECK();
    return 0;
  });
}

}  // extern "C"
