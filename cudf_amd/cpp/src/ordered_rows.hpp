// ordered_rows.hpp -- the key columns of one side of a call as the host arrays of the C ABI (merge, search, the selectors of the stream
// compaction), and what cudf::merge and cudf::lower_bound / upper_bound hand over besides: the per-key direction / null placement.
#pragma once
#include "common.hpp"

#include <cudf/table/table_view.hpp>

#include <vector>

namespace cudf {
namespace detail {

constexpr size_type MAX_KEYS = 32;  // key columns of one call (gx.h)

// of a table_view or a vector of column_views: the gx dtypes (cudf::data_type_error for a type the kernels do not take) ...
template <typename Columns>
std::vector<int> key_dtypes(Columns const& keys)
{
  std::vector<int> dtypes;
  for (auto const& c : keys) dtypes.push_back(gx_type(c.type()));
  return dtypes;
}
// ... and row 0's data pointers
template <typename Columns>
std::vector<void const*> key_data(Columns const& keys)
{
  std::vector<void const*> data;
  for (auto const& c : keys) data.push_back(row0(c));
  return data;
}

// sliced views: row 0's data pointer, the bitmap read from the view's offset on
struct key_side {
  std::vector<void const*> data;
  std::vector<uint32_t const*> valid;
  std::vector<int64_t> begin;
  int64_t rows;
  explicit key_side(table_view const& keys) : data{key_data(keys)}, rows{keys.num_rows()}
  {
    for (auto const& c : keys) {
      valid.push_back(c.has_nulls() ? c.null_mask() : nullptr);
      begin.push_back(c.offset());
    }
  }
};

struct key_order {
  std::vector<int> dtypes, descending, null_before;
  // the caller has checked the sizes: column_order one per key, null_precedence empty (= BEFORE) or one per key
  key_order(table_view const& keys, std::vector<order> const& column_order, std::vector<null_order> const& null_precedence)
    : dtypes{key_dtypes(keys)}
  {
    for (size_type k = 0; k < keys.num_columns(); ++k) {
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
