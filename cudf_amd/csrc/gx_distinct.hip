// gx_distinct.hip -- the deduplicating selectors of the ordered stream compaction: the kernels behind cudf::unique / distinct /
// stable_distinct / distinct_indices / distinct_count / unique_count (include/cudf/stream_compaction.hpp).
// Replaces the reference's reduction over a cuco static_set of row indices (src/stream_compaction/distinct.cu,
// distinct_helpers.cu, stable_distinct.cu, distinct_count.cu) and its adjacent-row copy_if (unique.cu, unique_count.cu).
//
// Both are SELECTORS in the sense of gx_compact.hpp: they write the plan (one bit per row + chunk starts) to the start of the
// caller's scratch and the number of selected rows to *count_dev; gx_compact_column / gx_compact_indices do the rest.
//
// unique    a streaming predicate: row i against row i - 1 and / or i + 1, through the key columns.
// distinct  a lock-free open-addressing table of ROW INDICES (rep[], int32, capacity = the power of two >= 2 n, empty = -1):
//             row i hashes its key row and probes linearly: r = atomicCAS(&rep[s], -1, i);
//               r == -1                      the row claimed the slot for its class;
//               row r equals row i           (compared through the key columns) the class's slot: atomicMin / atomicMax of the
//                                            row index (KEEP_FIRST, KEEP_NONE / KEEP_LAST), nothing under KEEP_ANY;
//               else                         the next slot.
//           A slot's CLASS never changes, whichever member's index it holds at the moment, so a comparison against a value that
//           has since been replaced is still a comparison against the right class.  No waits, no dependency between workgroups;
//           probing ends because at most n <= capacity / 2 slots are ever taken and none is freed.  All atomics are device scope.
//           KEEP_NONE keeps hi[] next to rep[]: every row that settles on a slot does atomicMax(&hi[s], i), so the class has one
//           member iff rep[s] == hi[s] (its min is its max).
//           KEEP_ANY is ONE pass: the insert is the predicate (selected iff the CAS claimed the slot) -- k_select_pred evaluates
//           every row exactly once.  The other options take two: the insert records slot_of[i], a second select kernel asks
//           rep[slot_of[i]] == i (and hi[...] == i).
//           Rows that can equal nothing (a null without "nulls equal", a NaN without "NaNs equal") never enter the table.
#include "gx_compact.hpp"

namespace gx {
namespace distinct {

using compact::MAX_KEYS;
using compact::Plan;

enum { F_NULLS_EQUAL = 1, F_NANS_EQUAL = 2, F_NAN_IS_NULL = 4, F_DROP_NULL_ROWS = 8, F_ALL = 15 };
enum { E_VALUE = 0, E_NULL = 1, E_NAN = 2 };

static std::atomic<int> g_hash_bits{0};  // test hook (gx_knobs.h): 0 = the whole hash, > 0 = its low bits, < 0 = none of it

struct Keys {
  rows::Cols<MAX_KEYS> c;
  int flags;

  // element k of row i as (E_ kind, bits): the element rules of gx_rows.hpp, with a NaN told apart (it is one value, or a null under
  // F_NAN_IS_NULL) because the flags decide what it equals
  __device__ __forceinline__ int load(int k, int64_t i, uint64_t& b) const
  {
    b = 0;
    if (!c.is_valid(k, i)) return E_NULL;
    b = c.bits(k, i);
    if (c.kind[k] == K_FLOAT) {
      const int w = c.width[k];
      if (rows::is_zero_elem(b, w)) b = 0;
      else if (rows::is_nan_elem(b, w)) {
        b = 0;
        return (flags & F_NAN_IS_NULL) ? E_NULL : E_NAN;
      }
    }
    return E_VALUE;
  }
  __device__ __forceinline__ bool equal(int64_t i, int64_t j) const
  {
    for (int k = 0; k < c.n; ++k) {
      uint64_t x, y;
      const int kx = load(k, i, x), ky = load(k, j, y);
      if (kx != ky || x != y) return false;
      if (kx == E_NULL && !(flags & F_NULLS_EQUAL)) return false;
      if (kx == E_NAN && !(flags & F_NANS_EQUAL)) return false;
    }
    return true;
  }
  // hash of row i; has_null / has_nan: an element of that kind is among its keys
  __device__ __forceinline__ uint64_t hash(int64_t i, bool& has_null, bool& has_nan) const
  {
    uint64_t h = 0x243F6A8885A308D3ull;
    has_null = has_nan = false;
    for (int k = 0; k < c.n; ++k) {
      uint64_t b;
      const int kind = load(k, i, b);
      if (kind == E_NULL) {
        has_null = true;
        b        = 0xA54FF53A5F1D36F1ull;  // every null element hashes alike
      } else if (kind == E_NAN) {
        has_nan = true;
        b       = 0x7FF8000000000000ull;
      }
      h = rows::fold_hash(h, b);
    }
    return h;
  }
};

// ---------------------------------------------------------------------------------------------- unique
struct UniquePred {
  Keys keys;
  int64_t n;
  int keep;
  __device__ __forceinline__ bool operator()(int64_t i) const
  {
    if (keys.flags & F_DROP_NULL_ROWS) {
      for (int k = 0; k < keys.c.n; ++k) {
        uint64_t b;
        if (keys.load(k, i, b) == E_NULL) return false;
      }
    }
    const bool first = i == 0 || !keys.equal(i, i - 1);
    if (keep == GX_KEEP_ANY || keep == GX_KEEP_FIRST) return first;
    const bool last = i == n - 1 || !keys.equal(i, i + 1);
    return keep == GX_KEEP_LAST ? last : (first && last);
  }
};

// ---------------------------------------------------------------------------------------------- distinct
struct Table {
  int32_t* rep;       // capacity slots: a row of the slot's class (the smallest / largest seen so far under KEEP_FIRST / KEEP_LAST), -1 = empty
  int32_t* hi;        // KEEP_NONE: the largest row of the slot's class
  uint32_t* slot_of;  // two-pass options: the slot row i settled on; for a row outside the table 1 = selected, 0 = not
  uint64_t* in_table;  // two-pass options: ballot words, bit = row i settled on a slot
  uint64_t mask;      // capacity - 1
  uint64_t hash_and;  // test hook: the bits of the hash that count
};

static inline uint64_t capacity_for(int64_t n)
{
  uint64_t c = 64;
  while (c < 2 * (uint64_t)n) c <<= 1;
  return c;
}
struct Layout {
  Plan plan;
  Table t;
  uint64_t capacity;
  size_t table_bytes;  // rep (+ hi): what the memset fills
  size_t bytes;
};
static inline Layout carve_all(const void* tmp, int64_t n, int keep)
{
  Layout l;
  l.plan     = compact::carve(tmp, n);
  l.capacity = capacity_for(n);
  Carver c(tmp ? const_cast<char*>(static_cast<const char*>(tmp)) + l.plan.bytes : nullptr);  // everything else lies behind the plan
  const size_t arrays = keep == GX_KEEP_NONE ? 2 : 1;
  l.t.rep       = c.take<int32_t>((size_t)l.capacity * arrays);
  l.t.hi        = (keep == GX_KEEP_NONE && l.t.rep) ? l.t.rep + l.capacity : nullptr;
  l.table_bytes = (size_t)l.capacity * arrays * sizeof(int32_t);
  l.t.slot_of   = nullptr;
  l.t.in_table  = nullptr;
  if (keep != GX_KEEP_ANY) {
    l.t.slot_of  = c.take<uint32_t>((size_t)n);
    l.t.in_table = c.take<uint64_t>((size_t)div_up(n, (int64_t)GX_WAVE) + 1);
  }
  l.t.mask     = l.capacity - 1;
  l.t.hash_and = ~0ull;
  l.bytes      = l.plan.bytes + c.total();
  return l;
}

// The insert of row i.  KEEP_ANY: returns "selected".  Otherwise: records where the row went, returns "it settled on a slot".
template <int KEEP>
struct InsertPred {
  Keys keys;
  Table t;
  __device__ __forceinline__ bool operator()(int64_t i) const
  {
    bool has_null, has_nan;
    const uint64_t h = keys.hash(i, has_null, has_nan);
    const bool dropped = has_null && (keys.flags & F_DROP_NULL_ROWS);
    const bool alone   = (has_null && !(keys.flags & F_NULLS_EQUAL)) || (has_nan && !(keys.flags & F_NANS_EQUAL));
    if (dropped || alone) {  // outside the table: a row that is not wanted, or one that equals no row
      if (KEEP == GX_KEEP_ANY) return !dropped;
      t.slot_of[i] = dropped ? 0u : 1u;
      return false;
    }
    const int32_t me = (int32_t)i;
    uint64_t s       = (h & t.hash_and) & t.mask;
    for (;;) {
      // a look before the CAS: a slot that was ever seen taken stays taken, by the same class
      int32_t r = __hip_atomic_load(&t.rep[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (r == -1) r = atomicCAS(&t.rep[s], -1, me);
      if (r == -1) {
        if (KEEP == GX_KEEP_NONE) atomicMax(&t.hi[s], me);
        break;
      }
      if (keys.equal(i, r)) {
        if (KEEP == GX_KEEP_ANY) return false;
        // rep[s] only falls (rises) from r on, so a row on the wrong side of r has nothing to add
        if ((KEEP == GX_KEEP_FIRST || KEEP == GX_KEEP_NONE) && me < r) atomicMin(&t.rep[s], me);
        if (KEEP == GX_KEEP_LAST && me > r) atomicMax(&t.rep[s], me);
        if (KEEP == GX_KEEP_NONE) atomicMax(&t.hi[s], me);
        break;
      }
      s = (s + 1) & t.mask;
    }
    if (KEEP == GX_KEEP_ANY) return true;
    t.slot_of[i] = (uint32_t)s;
    return true;
  }
};

template <int KEEP>
struct ResolvePred {
  Table t;
  __device__ __forceinline__ bool operator()(int64_t i) const
  {
    const uint32_t s = t.slot_of[i];
    if (!((t.in_table[i >> 6] >> (i & 63)) & 1ull)) return s != 0;
    const int32_t me = (int32_t)i;
    if (t.rep[s] != me) return false;
    return KEEP != GX_KEEP_NONE || t.hi[s] == me;
  }
};

template <int KEEP>
int two_pass(const Keys& keys, const Layout& l, int64_t n, int64_t* count_dev, hipStream_t s)
{
  // pass 1: the ballot of "settled on a slot" goes to in_table; the chunk counts it writes into the plan are overwritten by pass 2
  hipLaunchKernelGGL((compact::k_select_pred<InsertPred<KEEP>>), dim3((unsigned)l.plan.nchunks), dim3(256), 0, s, InsertPred<KEEP>{keys, l.t}, n,
                     l.t.in_table, l.plan.starts);
  GX_LAUNCH_CHECK();
  return compact::select_launch(ResolvePred<KEEP>{l.t}, n, l.plan, count_dev, s);
}

// arguments that both selectors share; fills `keys`
static int check_args(int nkeys, const int* dtypes_host, const void* const* cols_host, const uint32_t* const* valid_ptrs_host,
                      const int64_t* begin_bits_host, int64_t n, int keep, int flags, const void* sel_tmp, const size_t* tmp_bytes,
                      Keys& keys)
{
  if (compact::check_rows(n) || !tmp_bytes) return GX_EINVAL;
  if (keep < GX_KEEP_ANY || keep > GX_KEEP_NONE || flags < 0 || flags > F_ALL) return GX_EINVAL;
  keys.flags = flags;
  return rows::fill_cols(keys.c, nkeys, dtypes_host, cols_host, valid_ptrs_host, begin_bits_host, sel_tmp && n > 0);
}

static int zero_count(int64_t* count_dev, hipStream_t s)
{
  if (count_dev) GX_HIP_TRY(hipMemsetAsync(count_dev, 0, sizeof(int64_t), s));
  return 0;
}

}  // namespace distinct
}  // namespace gx

extern "C" {

using namespace gx;
using namespace gx::distinct;

void gx_distinct_set_hash_bits(int bits) { g_hash_bits.store(bits > 64 ? 0 : bits, std::memory_order_relaxed); }

int gx_select_unique(int nkeys, const int* dtypes_host, const void* const* cols_host, const uint32_t* const* valid_ptrs_host,
                     const int64_t* begin_bits_host, int64_t n, int keep, int flags, int64_t* count_dev, void* sel_tmp,
                     size_t* tmp_bytes, gx_stream_t stream)
{
  UniquePred pred{};
  if (int rc = check_args(nkeys, dtypes_host, cols_host, valid_ptrs_host, begin_bits_host, n, keep, flags, sel_tmp, tmp_bytes, pred.keys)) return rc;
  const Plan p = compact::carve(sel_tmp, n);
  if (int rc; !scratch_ready(sel_tmp, p.bytes, tmp_bytes, &rc)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) return zero_count(count_dev, s);
  pred.n    = n;
  pred.keep = keep;
  return compact::select_launch(pred, n, p, count_dev, s);
}

int gx_select_distinct(int nkeys, const int* dtypes_host, const void* const* cols_host, const uint32_t* const* valid_ptrs_host,
                       const int64_t* begin_bits_host, int64_t n, int keep, int flags, int64_t* count_dev, void* sel_tmp,
                       size_t* tmp_bytes, gx_stream_t stream)
{
  Keys keys;
  if (int rc = check_args(nkeys, dtypes_host, cols_host, valid_ptrs_host, begin_bits_host, n, keep, flags, sel_tmp, tmp_bytes, keys)) return rc;
  Layout l = carve_all(sel_tmp, n, keep);
  if (int rc; !scratch_ready(sel_tmp, l.bytes, tmp_bytes, &rc)) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (n == 0) return zero_count(count_dev, s);
  const int hb = g_hash_bits.load(std::memory_order_relaxed);
  l.t.hash_and = hb == 0 || hb >= 64 ? ~0ull : hb < 0 ? 0ull : ((1ull << hb) - 1ull);
  GX_HIP_TRY(hipMemsetAsync(l.t.rep, 0xFF, l.table_bytes, s));  // every slot (of rep and hi) = -1
  switch (keep) {
    case GX_KEEP_ANY: return compact::select_launch(InsertPred<GX_KEEP_ANY>{keys, l.t}, n, l.plan, count_dev, s);
    case GX_KEEP_FIRST: return two_pass<GX_KEEP_FIRST>(keys, l, n, count_dev, s);
    case GX_KEEP_LAST: return two_pass<GX_KEEP_LAST>(keys, l, n, count_dev, s);
    default: return two_pass<GX_KEEP_NONE>(keys, l, n, count_dev, s);
  }
}

}  // extern "C"
