// gx_merge.hip -- combining and searching what the sorts produce: the kernels behind cudf::merge and cudf::lower_bound / upper_bound
// (include/cudf/merge.hpp, include/cudf/search.hpp).  Replaces the reference's thrust::merge over a tagged row comparator
// (cpp/src/merge/merge.cu) and its thrust::lower_bound / upper_bound over the row comparator (cpp/src/search/search_ordered.cu).
//
// Row order: the lexicographic comparator of the multi-column sorts.  Per key column an element is (placement, sortable bits):
// sortable = rows::sortable_elem (gx_rows.hpp, where the element rules are stated) with the descending mask folded in, 0 for a null;
// placement = 1 for a valid element and 0 for a null when nulls come first (null_before != descending), the other way round when they
// come last.  Two rows compare column by column on that pair.
//
// merge (gx_merge_order), no key column with a bitmap on either side -- merge path, two launches:
//   k_mp_partition  one thread per tile: the split of its diagonal d = t * TILE, a_split[t] = the number of rows of A among the first d
//                   rows of the stable merge, found by a binary search of the cross-diagonal with the full row comparator.
//                   TIE RULE: on the diagonal A[i] is paired with B[d - 1 - i]; the search moves right (A[i] is among the first d) iff
//                   NOT (B[d-1-i] < A[i]), i.e. A[i] <= B[d-1-i].  "<=" for A, strict "<" for B: of two equivalent rows A's goes first.
//                   Turned round (A[i] < B[d-1-i] strictly) the same search would put B's equal rows first.
//   k_mp_merge      one workgroup per tile: the sortable leading keys of its A range and its B range (together exactly the tile's rows)
//                   staged in LDS, every thread finds the split of its own diagonal in LDS and merges ITEMS outputs serially; only when
//                   two leading keys agree and there are columns behind are those read from global memory.  The map leaves through LDS
//                   in whole lines.
//   Clamping: every binary search runs over [max(0, d - nb), min(d, na)], so both rows it compares exist whatever the data; a thread
//   merges between ITS split and its neighbour's, bounds checked on both sides.  For sorted input neighbouring splits are monotone by
//   the merge-path argument.  For unsorted input they need not be, so each level checks them (partition: every pair of neighbouring
//   tiles, a flag word; merge: every pair of neighbouring threads, a workgroup vote) and, where a pair is out of order, takes the
//   data-independent proportional split floor(d * na / (na + nb)) instead: monotone, inside the same bounds.  Hence the map is a
//   permutation of [0, na + nb) for ANY input, and the stable merge for sorted input.
// merge, some key column with a bitmap -- position by search (k_merge_by_search): row i of A goes to i + lower_bound(B, A[i]), row j of
//   B to j + upper_bound(A, B[j]): the same tie rule, the same comparator, no placement bits in LDS.  Both positions are < na + nb by
//   construction; the map is zeroed first, so unsorted input (whose positions may collide) still leaves only entries in range.
// search (gx_search_bounds): one needle per thread, a binary search over [0, n_hay) with lo <= mid < hi -- clamped by construction.
//   One key column without bitmaps: the needle's sortable form is computed once and the loop reads one haystack element per step.
// gx_gather2: out[i] = map[i] < na ? a[map[i]] : b[map[i] - na], validity likewise (a side without a bitmap is all valid); a map entry
//   outside [0, na + nb) reads nothing and gives a null / zero element.
#include "gx_rows.hpp"

namespace gx {
namespace merge {

constexpr int BT       = 256;         // threads of a tile workgroup
constexpr int ITEMS    = 8;           // outputs per thread
constexpr int TILE     = BT * ITEMS;  // outputs per workgroup: 16 KiB of leading keys in LDS, 8 workgroups (all 32 waves) per CU

using Side = rows::Cols<rows::MAX_KEYS>;  // one side's key columns
struct Meta {                              // the order of the rows; the two sides of a call agree in n, width and kind
  uint32_t desc;                           // bit k: column k descending
  uint32_t nulls_first;                    // bit k: null_before != descending
  int nkeys;
};

// element k of row i as sortable bits; place: see the header.  A null's bytes are not read.
template <bool NULLABLE>
__device__ __forceinline__ uint64_t elem(const Side& s, const Meta& m, int k, int64_t i, uint32_t& place)
{
  const uint32_t nf = (m.nulls_first >> k) & 1u;
  place             = nf;
  if (NULLABLE && !s.is_valid(k, i)) {
    place = nf ^ 1u;
    return 0;
  }
  return rows::sortable_elem(s.col[k], s.width[k], s.kind[k], ((m.desc >> k) & 1u) ? ~0ull : 0ull, i);
}

// row i of x against row j of y from column k0 on: < 0, 0, > 0
template <bool NULLABLE>
__device__ __forceinline__ int cmp_rows(const Side& x, int64_t i, const Side& y, int64_t j, const Meta& m, int k0)
{
  for (int k = k0; k < m.nkeys; ++k) {
    uint32_t px, py;
    const uint64_t a = elem<NULLABLE>(x, m, k, i, px), b = elem<NULLABLE>(y, m, k, j, py);
    if (px != py) return px < py ? -1 : 1;
    if (a != b) return a < b ? -1 : 1;
  }
  return 0;
}

// the number of rows of `hay` that compare < (upper: <=) row `r` of `needle`: lo <= mid < hi <= n_hay at every step
template <bool NULLABLE>
__device__ __forceinline__ int32_t bound(const Side& hay, int64_t n_hay, const Side& needle, int64_t r, const Meta& m, bool upper)
{
  int64_t lo = 0, hi = n_hay;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    const int c       = cmp_rows<NULLABLE>(hay, mid, needle, r, m, 0);
    const bool right  = upper ? c <= 0 : c < 0;
    lo                = right ? mid + 1 : lo;
    hi                = right ? hi : mid;
  }
  return (int32_t)lo;
}

// ---------------------------------------------------------------------------------------------- search
template <bool NULLABLE>
__global__ void __launch_bounds__(256) k_search_bounds(Side hay, int64_t n_hay, Side needles, int64_t n_needles, Meta m, int upper,
                                                      int32_t* __restrict__ out)
{
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_needles) return;
  if (!NULLABLE && m.nkeys == 1) {  // the sortable form only: one haystack element per step
    uint32_t p;
    const uint64_t key = elem<false>(needles, m, 0, r, p);
    int64_t lo = 0, hi = n_hay;
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      const uint64_t h  = elem<false>(hay, m, 0, mid, p);
      const bool right  = upper ? h <= key : h < key;
      lo                = right ? mid + 1 : lo;
      hi                = right ? hi : mid;
    }
    out[r] = (int32_t)lo;
    return;
  }
  out[r] = bound<NULLABLE>(hay, n_hay, needles, r, m, upper != 0);
}

// ---------------------------------------------------------------------------------------------- merge by search (nullable keys)
__global__ void __launch_bounds__(256) k_merge_by_search(Side A, Side B, Meta m, int64_t na, int64_t nb, int32_t* __restrict__ out)
{
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= na + nb) return;
  // g - na + upper_bound <= (nb - 1) + na and g + lower_bound <= (na - 1) + nb: inside the map whatever the data
  const int64_t pos = g < na ? g + bound<true>(B, nb, A, g, m, false) : (g - na) + bound<true>(A, na, B, g - na, m, true);
  out[pos]          = (int32_t)g;
}

// ---------------------------------------------------------------------------------------------- merge path
// the data-independent split of diagonal d of (na, nb): monotone in d, steps of at most the step of d, inside [max(0, d - nb), min(d, na)]
__host__ __device__ __forceinline__ int64_t proportional_split(int64_t d, int64_t na, int64_t n) { return n > 0 ? d * na / n : 0; }

// the split of diagonal d: the number of rows of A among the first d rows of the stable merge.  See TIE RULE in the header.
__device__ __forceinline__ int64_t diagonal_split(const Side& A, const Side& B, const Meta& m, int64_t na, int64_t nb, int64_t d)
{
  int64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);  // lo <= mid < hi: 0 <= mid < na and 0 <= d - 1 - mid < nb
    const bool a_first = cmp_rows<false>(B, d - 1 - mid, A, mid, m, 0) >= 0;  // NOT (B < A): A[mid] <= B[d - 1 - mid]
    lo                 = a_first ? mid + 1 : lo;
    hi                 = a_first ? hi : mid;
  }
  return lo;
}

__global__ void __launch_bounds__(256) k_mp_partition(Side A, Side B, Meta m, int64_t na, int64_t nb, int64_t ntiles, int32_t* __restrict__ a_split,
                                                     uint32_t* __restrict__ flag)
{
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= ntiles) return;
  const int64_t n = na + nb, d0 = t * TILE, d1 = d0 + TILE < n ? d0 + TILE : n;
  const int64_t s0 = t == 0 ? 0 : diagonal_split(A, B, m, na, nb, d0);
  const int64_t s1 = d1 == n ? na : diagonal_split(A, B, m, na, nb, d1);  // what the next thread finds for itself
  a_split[t]       = (int32_t)s0;
  if (s1 < s0 || s1 - s0 > d1 - d0) atomicOr(flag, 1u);  // neighbouring splits out of order: the input was not sorted
}

__global__ void __launch_bounds__(BT) k_mp_merge(Side A, Side B, Meta m, int64_t na, int64_t nb, const int32_t* __restrict__ a_split,
                                                 const uint32_t* __restrict__ flag, int32_t* __restrict__ out)
{
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint64_t* s_key = reinterpret_cast<uint64_t*>(smem);                     // [0, ac): A's leading keys, [ac, cnt): B's
  int32_t* s_out  = reinterpret_cast<int32_t*>(smem);                      // the map, once the keys are done with
  int32_t* s_split = reinterpret_cast<int32_t*>(smem + (size_t)TILE * 8);  // BT + 1 thread splits
  const int tid   = threadIdx.x;
  const int64_t n = na + nb, t = blockIdx.x;
  const int64_t d0 = t * TILE, d1 = d0 + TILE < n ? d0 + TILE : n;
  const int cnt    = (int)(d1 - d0);
  const bool unsorted = *flag != 0;  // wave-uniform
  const int64_t a0 = unsorted ? proportional_split(d0, na, n) : (t == 0 ? 0 : (int64_t)a_split[t]);
  const int64_t a1 = unsorted ? proportional_split(d1, na, n) : (d1 == n ? na : (int64_t)a_split[t + 1]);
  const int64_t b0 = d0 - a0;
  const int ac = (int)(a1 - a0), bc = cnt - ac;  // 0 <= ac <= cnt: checked by k_mp_partition, or proportional

  for (int i = tid; i < cnt; i += BT) {
    uint32_t p;
    s_key[i] = i < ac ? elem<false>(A, m, 0, a0 + i, p) : elem<false>(B, m, 0, b0 + (i - ac), p);
  }
  if (tid == 0) s_split[BT] = ac;
  __syncthreads();

  // A's local row i against B's local row j: does A's go first?  (the columns behind only on a tie of the leading keys)
  auto a_first = [&](uint64_t ka, int i, uint64_t kb, int j) -> bool {
    if (ka != kb) return ka < kb;
    return m.nkeys == 1 || cmp_rows<false>(B, b0 + j, A, a0 + i, m, 1) >= 0;
  };
  const int di = tid * ITEMS < cnt ? tid * ITEMS : cnt, dn = di + ITEMS < cnt ? di + ITEMS : cnt;
  {
    int lo = di > bc ? di - bc : 0, hi = di < ac ? di : ac;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;  // 0 <= mid < ac and 0 <= di - 1 - mid < bc
      const bool af = a_first(s_key[mid], mid, s_key[ac + (di - 1 - mid)], di - 1 - mid);
      lo            = af ? mid + 1 : lo;
      hi            = af ? hi : mid;
    }
    s_split[tid] = lo;
  }
  __syncthreads();
  int ai = s_split[tid], an = s_split[tid + 1];
  if (__syncthreads_or(an < ai || an - ai > dn - di)) {  // unsorted rows inside the tile: the proportional split of the tile
    ai = cnt > 0 ? (int)((int64_t)di * ac / cnt) : 0;
    an = cnt > 0 ? (int)((int64_t)dn * ac / cnt) : 0;
  }
  // this thread's outputs: rows [ai, an) of the A range and [di - ai, dn - an) of the B range, nothing else
  int i = ai, j = di - ai;
  const int iend = an, jend = dn - an;
  uint64_t ka = i < iend ? s_key[i] : 0, kb = j < jend ? s_key[ac + j] : 0;
  int32_t r[ITEMS];
#pragma unroll
  for (int u = 0; u < ITEMS; ++u) {
    r[u] = 0;
    if (di + u < dn) {
      const bool take_a = j >= jend || (i < iend && a_first(ka, i, kb, j));
      if (take_a) {
        r[u] = (int32_t)(a0 + i);
        ++i;
        ka = i < iend ? s_key[i] : 0;
      } else {
        r[u] = (int32_t)(na + b0 + j);
        ++j;
        kb = j < jend ? s_key[ac + j] : 0;
      }
    }
  }
  __syncthreads();  // every thread is done with the keys
#pragma unroll
  for (int u = 0; u < ITEMS; ++u)
    if (di + u < dn) s_out[di + u] = r[u];
  __syncthreads();
  for (int k = tid; k < cnt; k += BT) out[d0 + k] = s_out[k];
}

// ---------------------------------------------------------------------------------------------- gather from two sources
template <typename T>
__global__ void __launch_bounds__(256) k_gather2(const T* __restrict__ a, const uint32_t* __restrict__ a_valid, int64_t a_bit0, int64_t na,
                                                const T* __restrict__ b, const uint32_t* __restrict__ b_valid, int64_t b_bit0, int64_t nb,
                                                const int32_t* __restrict__ map, int64_t n, T* __restrict__ out, uint32_t* __restrict__ out_valid,
                                                unsigned long long* __restrict__ null_count)
{
  constexpr int ROUNDS = 4;  // 1024 rows per workgroup, a wave owns whole 64-row groups (two validity words)
  const int64_t base   = (int64_t)blockIdx.x * (256 * ROUNDS);
  uint32_t nulls       = 0;
#pragma unroll
  for (int r = 0; r < ROUNDS; ++r) {
    const int64_t row = base + r * 256 + threadIdx.x;
    bool ok           = false;
    if (row < n) {
      const uint32_t mrow = (uint32_t)map[row];
      T v                 = T(0);
      if ((int64_t)mrow < na) {
        ok = a_valid == nullptr || bit_is_set(a_valid, a_bit0 + mrow);
        v  = a[mrow];
      } else if ((int64_t)mrow < na + nb) {
        const int64_t j = (int64_t)mrow - na;
        ok              = b_valid == nullptr || bit_is_set(b_valid, b_bit0 + j);
        v               = b[j];
      }
      out[row] = v;
    }
    if (out_valid) {  // (wave-uniform)
      const uint64_t bal = store_wave_validity(out_valid, row & ~(int64_t)63, n, ok);
      if (lane_id() == 0) {
        const int64_t first = row, left = n - first;  // lane 0's row is the group's first
        const int live      = left >= 64 ? 64 : (left > 0 ? (int)left : 0);
        nulls += (uint32_t)(live - __builtin_popcountll(bal));
      }
    }
  }
  if (null_count && nulls) atomicAdd(null_count, (unsigned long long)nulls);
}

// ---------------------------------------------------------------------------------------------- host
static Meta fill_meta(int nkeys, const int* descending, const int* null_before)
{
  Meta m{};
  m.nkeys = nkeys;
  for (int k = 0; k < nkeys; ++k) {
    const bool desc = descending && descending[k] != 0, before = !null_before || null_before[k] != 0;
    if (desc) m.desc |= 1u << k;
    if (before != desc) m.nulls_first |= 1u << k;
  }
  return m;
}

struct Scratch {
  int32_t* a_split;
  uint32_t* flag;
  size_t bytes;
};
static Scratch carve(void* tmp, int64_t n)
{
  Carver c(tmp);
  Scratch s;
  s.a_split = c.take<int32_t>((size_t)div_up(n, (int64_t)TILE) + 1);
  s.flag    = c.take<uint32_t>(1);
  s.bytes   = c.total();
  return s;
}

template <typename T>
static void launch_gather2(const void* a, const uint32_t* av, int64_t abit, int64_t na, const void* b, const uint32_t* bv, int64_t bbit, int64_t nb,
                           const int32_t* map, int64_t n, void* out, uint32_t* out_valid, int64_t* nulls, hipStream_t s)
{
  hipLaunchKernelGGL(k_gather2<T>, dim3((unsigned)div_up(n, (int64_t)1024)), dim3(256), 0, s, static_cast<const T*>(a), av, abit, na,
                     static_cast<const T*>(b), bv, bbit, nb, map, n, static_cast<T*>(out), out_valid, reinterpret_cast<unsigned long long*>(nulls));
}

}  // namespace merge
}  // namespace gx

extern "C" {

using namespace gx;
using namespace gx::merge;

int gx_merge_tile_rows(void) { return TILE; }

int gx_merge_order(int nkeys, const int* dtypes_host, const void* const* a_cols_host, const uint32_t* const* a_valid_ptrs_host,
                   const int64_t* a_begin_bits_host, int64_t na, const void* const* b_cols_host, const uint32_t* const* b_valid_ptrs_host,
                   const int64_t* b_begin_bits_host, int64_t nb, const int* descending_host, const int* null_before_host, int32_t* out_map, void* tmp,
                   size_t* tmp_bytes, gx_stream_t stream)
{
  if (!tmp_bytes || na < 0 || nb < 0 || na > 0x7FFFFFFFll || nb > 0x7FFFFFFFll || na + nb > 0x7FFFFFFFll) return GX_EINVAL;
  const int64_t n      = na + nb;
  const bool launching = tmp != nullptr && n > 0;
  Side A, B;  // pointers are only demanded when the side has rows and the call will launch
  if (int rc = rows::fill_cols(A, nkeys, dtypes_host, a_cols_host, a_valid_ptrs_host, a_begin_bits_host, launching && na > 0)) return rc;
  if (int rc = rows::fill_cols(B, nkeys, dtypes_host, b_cols_host, b_valid_ptrs_host, b_begin_bits_host, launching && nb > 0)) return rc;
  const Meta m        = fill_meta(nkeys, descending_host, null_before_host);
  const bool nullable = A.has_bitmaps() || B.has_bitmaps();
  const Scratch sc = carve(tmp, n);
  if (int rc; !gx::scratch_ready(tmp, sc.bytes, tmp_bytes, &rc)) return rc;
  if (n == 0) return 0;
  if (!out_map) return GX_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (nullable) {
    GX_HIP_TRY(hipMemsetAsync(out_map, 0, (size_t)n * sizeof(int32_t), s));
    hipLaunchKernelGGL(k_merge_by_search, dim3((unsigned)div_up(n, (int64_t)256)), dim3(256), 0, s, A, B, m, na, nb, out_map);
    GX_LAUNCH_CHECK();
    return 0;
  }
  Device dev;
  GX_HIP_TRY(device(&dev));
  const int64_t ntiles = div_up(n, (int64_t)TILE);
  GX_HIP_TRY(hipMemsetAsync(sc.flag, 0, sizeof(uint32_t), s));
  hipLaunchKernelGGL(k_mp_partition, dim3((unsigned)div_up(ntiles, (int64_t)256)), dim3(256), 0, s, A, B, m, na, nb, ntiles, sc.a_split, sc.flag);
  GX_HIP_TRY(launch_lds(dev, k_mp_merge, dim3((unsigned)ntiles), dim3(BT), (size_t)TILE * 8 + align_up((BT + 1) * 4, 16), s, A, B, m, na, nb,
                        (const int32_t*)sc.a_split, (const uint32_t*)sc.flag, out_map));
  GX_LAUNCH_CHECK();
  return 0;
}

int gx_search_bounds(int nkeys, const int* dtypes_host, const void* const* hay_cols_host, const uint32_t* const* hay_valid_ptrs_host,
                     const int64_t* hay_begin_bits_host, int64_t n_hay, const void* const* needle_cols_host,
                     const uint32_t* const* needle_valid_ptrs_host, const int64_t* needle_begin_bits_host, int64_t n_needles,
                     const int* descending_host, const int* null_before_host, int upper, int32_t* out, gx_stream_t stream)
{
  if (n_hay < 0 || n_needles < 0 || n_hay > 0x7FFFFFFFll || n_needles > 0x7FFFFFFFll) return GX_EINVAL;
  Side H, N;
  if (int rc = rows::fill_cols(H, nkeys, dtypes_host, hay_cols_host, hay_valid_ptrs_host, hay_begin_bits_host, n_needles > 0 && n_hay > 0)) return rc;
  if (int rc = rows::fill_cols(N, nkeys, dtypes_host, needle_cols_host, needle_valid_ptrs_host, needle_begin_bits_host, n_needles > 0)) return rc;
  const Meta m        = fill_meta(nkeys, descending_host, null_before_host);
  const bool nullable = H.has_bitmaps() || N.has_bitmaps();
  if (n_needles == 0) return 0;
  if (!out) return GX_EINVAL;
  hipStream_t s       = (hipStream_t)stream;
  const unsigned grid = (unsigned)div_up(n_needles, (int64_t)256);
  if (nullable) hipLaunchKernelGGL(k_search_bounds<true>, dim3(grid), dim3(256), 0, s, H, n_hay, N, n_needles, m, upper ? 1 : 0, out);
  else hipLaunchKernelGGL(k_search_bounds<false>, dim3(grid), dim3(256), 0, s, H, n_hay, N, n_needles, m, upper ? 1 : 0, out);
  GX_LAUNCH_CHECK();
  return 0;
}

int gx_gather2(int elem_size, const void* a, const uint32_t* a_valid, int64_t a_begin_bit, int64_t na, const void* b, const uint32_t* b_valid,
               int64_t b_begin_bit, int64_t nb, const int32_t* map, int64_t n, void* out, uint32_t* out_valid, int64_t* out_null_count_dev,
               gx_stream_t stream)
{
  if (na < 0 || nb < 0 || n < 0 || na + nb > 0x7FFFFFFFll || n > 0x7FFFFFFFll || a_begin_bit < 0 || b_begin_bit < 0) return GX_EINVAL;
  if (elem_size != 1 && elem_size != 2 && elem_size != 4 && elem_size != 8) return GX_EDTYPE;
  if ((a_valid || b_valid) && !out_valid) return GX_EINVAL;
  if (n > 0 && (!map || !out || (na > 0 && !a) || (nb > 0 && !b))) return GX_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (out_null_count_dev) GX_HIP_TRY(hipMemsetAsync(out_null_count_dev, 0, sizeof(int64_t), s));
  if (n == 0) return 0;
  return with_width(elem_size, [&](auto tag) {
    launch_gather2<decltype(tag)>(a, a_valid, a_begin_bit, na, b, b_valid, b_begin_bit, nb, map, n, out, out_valid, out_null_count_dev, s);
    GX_LAUNCH_CHECK();
    return 0;
  });
}

}  // extern "C"
