// ordered_rows.hpp -- what cudf::merge and cudf::lower_bound / upper_bound hand to gx_merge_order / gx_search_bounds: the key columns
// of one side as the host arrays of the C ABI, and the per-key direction / null placement.
#pragma once
#include "common.hpp"

#include <cudf/table/table_view.hpp>

#include <vector>

namespace cudf {
namespace detail {

constexpr size_type MAX_ORDERED_KEYS = 32;  // key columns of one call (gx.h)

// sliced views: row 0's data pointer, the bitmap read from the view's offset on
struct key_side {
  std::vector<void const*> data;
  std::vector<uint32_t const*> valid;
  std::vector<int64_t> begin;
  int64_t rows;
  explicit key_side(table_view const& keys) : rows{keys.num_rows()}
  {
    for (auto const& c : keys) {
      data.push_back(row0(c));
      valid.push_back(c.has_nulls() ? c.null_mask() : nullptr);
      begin.push_back(c.offset());
    }
  }
};

struct key_order {
  std::vector<int> dtypes, descending, null_before;
  // the caller has checked the sizes: column_order one per key, null_precedence empty (= BEFORE) or one per key
  key_order(table_view const& keys, std::vector<order> const& column_order, std::vector<null_order> const& null_precedence)
  {
    for (size_type k = 0; k < keys.num_columns(); ++k) {
      dtypes.push_back(gx_type(keys.column(k).type()));
      descending.push_back(column_order[k] == order::DESCENDING ? 1 : 0);
      null_before.push_back(null_precedence.empty() || null_precedence[k] == null_order::BEFORE ? 1 : 0);
    }
  }
};

inline bool same_types(table_view const& a, table_view const& b)
{
  if (a.num_columns() != b.num_columns()) return false;
  for (size_type k = 0; k < a.num_columns(); ++k)
    if (a.column(k).type() != b.column(k).type()) return false;
  return true;
}

}  // namespace detail
}  // namespace cudf
