// gx_dtype.hpp -- the one table from a gx_dtype to the types and constants a host dispatch picks a kernel instantiation by.
// Plain C++ (no HIP include), so the host tests read it too (tests/cpp/cudf_host_tests.cpp).
#pragma once

#include <stdint.h>

#include <type_traits>

#include "../../include/cudf_amd/gx.h"

namespace gx {

// how a key's bits order (to_sortable, gx_common.hpp); K_FTOTAL is the sort's own choice for clean float columns, never a dtype's
enum KeyKind { K_UNSIGNED = 0, K_SIGNED = 1, K_FLOAT = 2, K_FTOTAL = 3 };

// One row of the table: value_type is the element as arithmetic sees it, word_type the unsigned word of its width (what the key
// kernels load), kind how those bits order, is_bool the one dtype whose nonzero bytes all mean `true`.
template <typename V, typename W, KeyKind KIND, bool BOOL = false>
struct DType {
  using value_type = V;
  using word_type  = W;
  static constexpr KeyKind kind = KIND;
  static constexpr bool is_bool = BOOL;
};

// what a kernel that treats integers of either sign alike is instantiated with: the word for integers, the value type for floats
template <typename D>
using word_or_float_t = std::conditional_t<D::kind == K_FLOAT, typename D::value_type, typename D::word_type>;

// f(DType<...>{}) for the row of `dtype`, and f's return code; GX_EDTYPE, and no call, for any other value.  f is a generic
// callable: `[&](auto t) { using D = decltype(t); ... }`.
template <typename F>
inline int with_dtype(int dtype, F&& f)
{
  switch (dtype) {
    case GX_INT8: return f(DType<int8_t, uint8_t, K_SIGNED>{});
    case GX_INT16: return f(DType<int16_t, uint16_t, K_SIGNED>{});
    case GX_INT32: return f(DType<int32_t, uint32_t, K_SIGNED>{});
    case GX_INT64: return f(DType<int64_t, uint64_t, K_SIGNED>{});
    case GX_UINT8: return f(DType<uint8_t, uint8_t, K_UNSIGNED>{});
    case GX_UINT16: return f(DType<uint16_t, uint16_t, K_UNSIGNED>{});
    case GX_UINT32: return f(DType<uint32_t, uint32_t, K_UNSIGNED>{});
    case GX_UINT64: return f(DType<uint64_t, uint64_t, K_UNSIGNED>{});
    case GX_BOOL8: return f(DType<uint8_t, uint8_t, K_UNSIGNED, true>{});
    case GX_FLOAT32: return f(DType<float, uint32_t, K_FLOAT>{});
    case GX_FLOAT64: return f(DType<double, uint64_t, K_FLOAT>{});
    default: return GX_EDTYPE;
  }
}

}  // namespace gx
