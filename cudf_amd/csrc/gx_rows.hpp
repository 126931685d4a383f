// gx_rows.hpp -- how a kernel looks at one element of a key column.  Every operator that sees a row through its key columns (row keys
// and hashes: gx_rank.hip; distinct / unique: gx_distinct.hip; merge and search: gx_merge.hip; the tuple sort: gx_order.hip; the row
// filters: gx_compact.hip) reads its elements through this header, so the rules are stated once:
//   * an element is its bytes zero-extended to 64 bits (load_bits): 1, 2, 4 or 8 bytes wide;
//   * a column's bitmap (NULL = no nulls) is read from bit0 + i, and a null's bytes are never read;
//   * EQUALITY of floats is that of the row comparator (detail/row_operator/common_utils.cuh:215-220): -0.0 == +0.0 and every NaN is
//     one value -- normalise_float maps each class to one bit pattern (integers need nothing);
//   * ORDER is the unsigned order of to_sortable (gx_common.hpp) -- sortable_elem; equal sortable bits <=> equal normalised bits.
// Outside gx_common.hpp and gx_sort.hip the exponent masks of the float formats appear here only.
#pragma once
#include "gx_common.hpp"

namespace gx {
namespace rows {

constexpr int MAX_KEYS = 32;  // key columns of one call (the row-key calls of gx_rank.hip and the tuple sort take 8)

__device__ __forceinline__ uint64_t load_bits(const void* p, int width, int64_t i)
{
  switch (width) {
    case 1: return static_cast<const uint8_t*>(p)[i];
    case 2: return static_cast<const uint16_t*>(p)[i];
    case 4: return static_cast<const uint32_t*>(p)[i];
    default: return static_cast<const uint64_t*>(p)[i];
  }
}

// ---- float classes, on the bits (U = uint32_t / uint64_t)
template <typename U>
__host__ __device__ __forceinline__ bool is_nan_bits(U b)
{
  constexpr U EXP = (sizeof(U) == 8) ? U(0x7FF0000000000000ull) : U(0x7F800000u);
  return U(b & (U(~U(0)) >> 1)) > EXP;
}
template <typename U>
__host__ __device__ __forceinline__ bool is_zero_bits(U b)
{
  return U(b & (U(~U(0)) >> 1)) == 0;
}
// the same for a zero-extended element of `width` 4 or 8
__host__ __device__ __forceinline__ bool is_nan_elem(uint64_t b, int width) { return width == 4 ? is_nan_bits((uint32_t)b) : is_nan_bits(b); }
__host__ __device__ __forceinline__ bool is_zero_elem(uint64_t b, int width) { return width == 4 ? is_zero_bits((uint32_t)b) : is_zero_bits(b); }

// one bit pattern per equality class: +-0 -> 0, NaN -> the quiet NaN of the width
__host__ __device__ __forceinline__ uint64_t normalise_float(uint64_t b, int width)
{
  if (is_zero_elem(b, width)) return 0;
  if (is_nan_elem(b, width)) return width == 4 ? 0x7FC00000ull : 0x7FF8000000000000ull;
  return b;
}

// element i in sortable form, zero-extended; desc_mask = 0, or all ones for a descending column (only the column's width of it counts)
template <typename U>
__device__ __forceinline__ uint64_t sortable_int(const void* p, int kind, uint64_t desc_mask, int64_t i)
{
  const U b = static_cast<const U*>(p)[i];
  const U m = (U)desc_mask;
  if (kind == K_SIGNED) return (uint64_t)to_sortable<U, K_SIGNED>(b, m);
  return (uint64_t)to_sortable<U, K_UNSIGNED>(b, m);
}
__device__ __forceinline__ uint64_t sortable_elem(const void* p, int width, int kind, uint64_t desc_mask, int64_t i)
{
  switch (width) {
    case 8:
      if (kind == K_FLOAT) return to_sortable<uint64_t, K_FLOAT>(static_cast<const uint64_t*>(p)[i], desc_mask);
      return sortable_int<uint64_t>(p, kind, desc_mask, i);
    case 4:
      if (kind == K_FLOAT) return (uint64_t)to_sortable<uint32_t, K_FLOAT>(static_cast<const uint32_t*>(p)[i], (uint32_t)desc_mask);
      return sortable_int<uint32_t>(p, kind, desc_mask, i);
    case 2: return sortable_int<uint16_t>(p, kind, desc_mask, i);
    default: return sortable_int<uint8_t>(p, kind, desc_mask, i);
  }
}

// ---- the row hash: one fmix64 (MurmurHash3's 64-bit finaliser) per element, folded over the columns
__host__ __device__ __forceinline__ uint64_t fmix64(uint64_t x)
{
  x ^= x >> 33;
  x *= 0xFF51AFD7ED558CCDull;
  x ^= x >> 33;
  x *= 0xC4CEB9FE1A85EC53ull;
  x ^= x >> 33;
  return x;
}
__host__ __device__ __forceinline__ uint64_t fold_hash(uint64_t h, uint64_t elem_bits)
{
  return fmix64(h + 0x9E3779B97F4A7C15ull + elem_bits) ^ (h << 1 | h >> 63);
}

// ---- the key columns of one side of a call (sliced views: col = row 0, the bitmap read from bit0 on), passed to kernels by value
template <int N>
struct Cols {
  const void* col[N];
  const uint32_t* valid[N];  // NULL = a column without a bitmap
  int64_t bit0[N];
  int width[N];  // bytes (int, not a byte: a kernel argument indexed by k is then read by a scalar load)
  int kind[N];   // KeyKind
  int n;

  __device__ __forceinline__ bool is_valid(int k, int64_t i) const { return !valid[k] || bit_is_set(valid[k], bit0[k] + i); }
  __device__ __forceinline__ uint64_t bits(int k, int64_t i) const { return load_bits(col[k], width[k], i); }
  // the element's equality class as bits (the bitmap is the caller's business)
  __device__ __forceinline__ uint64_t normalised(int k, int64_t i) const
  {
    const uint64_t b = bits(k, i);
    return kind[k] == K_FLOAT ? normalise_float(b, width[k]) : b;
  }
  bool has_bitmaps() const
  {
    for (int k = 0; k < n; ++k)
      if (valid[k]) return true;
    return false;
  }
};

// ---- host: a dtype's row of the table (gx_dtype.hpp) as the runtime values Cols carries, and the argument rules of every call
// that takes key columns
inline int key_kind_width(int dtype, int* kind, int* width)
{
  return with_dtype(dtype, [&](auto t) {
    *kind  = decltype(t)::kind;
    *width = (int)sizeof(typename decltype(t)::word_type);
    return 0;
  });
}

// Fills `c` from the host arrays of a call: 1 <= nkeys <= N and `dtypes` are demanded, an unknown dtype is GX_EDTYPE, `bits` (NULL =
// all 0) must not be negative.  The pointers are demanded -- and stored -- only with need_ptrs: when the call will launch and the side
// has rows.  A NULL `valid` array means no bitmaps.
template <int N>
inline int fill_cols(Cols<N>& c, int nkeys, const int* dtypes, const void* const* cols, const uint32_t* const* valid, const int64_t* bits,
                     bool need_ptrs)
{
  if (nkeys < 1 || nkeys > N || !dtypes) return GX_EINVAL;
  c   = Cols<N>{};
  c.n = nkeys;
  for (int k = 0; k < nkeys; ++k) {
    int kind, width;
    if (key_kind_width(dtypes[k], &kind, &width)) return GX_EDTYPE;
    c.kind[k]  = kind;
    c.width[k] = width;
    c.bit0[k]  = bits ? bits[k] : 0;
    if (c.bit0[k] < 0) return GX_EINVAL;
  }
  if (!need_ptrs) return 0;
  if (!cols) return GX_EINVAL;
  for (int k = 0; k < nkeys; ++k) {
    if (!cols[k]) return GX_EINVAL;
    c.col[k]   = cols[k];
    c.valid[k] = valid ? valid[k] : nullptr;
  }
  return 0;
}

}  // namespace rows
}  // namespace gx
