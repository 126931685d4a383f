// cudf::merge over the C ABI (gx_merge_order -> gx_gather2 per column; cudf_amd/csrc/gx_merge.hip).
// reference: cpp/include/cudf/merge.hpp, cpp/src/merge/merge.cu -- there a thrust::merge of tagged row indices under the row
// comparator, then a two-source gather per column, repeated over a queue of tables.  Here: the merge map of two tables from the
// merge-path kernels (position by search when a key column has nulls), one gx_gather2 per column, and a balanced tree over
// NEIGHBOURING tables, so that rows that compare equivalent stay ordered by (table index, row).
// Stream-ordered.  Nothing is read back unless an input column has a null mask: then the null counts of a merge step's output
// columns come back in one read behind its gathers, which is what lets a column without nulls come back without a mask.
#include "common.hpp"
#include "ordered_rows.hpp"

#include <cudf/column/column_factories.hpp>
#include <cudf/merge.hpp>
#include <cudf/null_mask.hpp>

#include <limits>
#include <stdexcept>

namespace cudf {
namespace {

// a (sorted) and b (sorted), both with rows: the stable merge, a's rows first among equivalent ones
std::unique_ptr<table> merge_two(table_view const& a, table_view const& b, std::vector<size_type> const& key_cols,
                                 std::vector<order> const& column_order, std::vector<null_order> const& null_precedence,
                                 rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  auto const ka = a.select(key_cols), kb = b.select(key_cols);
  detail::key_order const ko{ka, column_order, null_precedence};
  detail::key_side const sa{ka}, sb{kb};
  auto const na = a.num_rows(), nb = b.num_rows();
  auto const n  = na + nb;
  rmm::device_uvector<int32_t> map(static_cast<std::size_t>(n), stream);
  auto scratch = detail::run_with_scratch(
    [&](void* t, std::size_t* bytes) {
      return gx_merge_order(static_cast<int>(ko.dtypes.size()), ko.dtypes.data(), sa.data.data(), sa.valid.data(), sa.begin.data(), na,
                            sb.data.data(), sb.valid.data(), sb.begin.data(), nb, ko.descending.data(), ko.null_before.data(), map.data(), t,
                            bytes, detail::gxs(stream));
    },
    "merge", stream);

  auto const nc = a.num_columns();
  rmm::device_uvector<int64_t> nulls_dev(static_cast<std::size_t>(nc), stream);
  std::vector<rmm::device_buffer> data, masks;
  data.reserve(nc);
  masks.reserve(nc);
  bool any_mask = false;
  for (size_type k = 0; k < nc; ++k) {
    auto const& ca = a.column(k);
    auto const& cb = b.column(k);
    auto const esz = static_cast<int>(size_of(ca.type()));
    bool const with_mask = ca.has_nulls() || cb.has_nulls();
    any_mask |= with_mask;
    data.emplace_back(static_cast<std::size_t>(n) * esz, stream, mr);
    masks.emplace_back(create_null_mask(n, with_mask ? mask_state::ALL_NULL : mask_state::UNALLOCATED, stream, mr));
    detail::gx_check(gx_gather2(esz, detail::row0(ca), ca.has_nulls() ? ca.null_mask() : nullptr, ca.offset(), na, detail::row0(cb),
                                cb.has_nulls() ? cb.null_mask() : nullptr, cb.offset(), nb, map.data(), n, data.back().data(),
                                with_mask ? static_cast<uint32_t*>(masks.back().data()) : nullptr, with_mask ? nulls_dev.data() + k : nullptr,
                                detail::gxs(stream)),
                     "gx_gather2");
  }
  std::vector<int64_t> nulls(static_cast<std::size_t>(nc), 0);
  if (any_mask) {
    // (columns without a mask left their word unwritten: only the words of masked columns are used below)
    CUDF_CUDA_TRY(hipMemcpyAsync(nulls.data(), nulls_dev.data(), nulls.size() * sizeof(int64_t), hipMemcpyDeviceToHost, stream.value()));
    stream.synchronize();
  }
  std::vector<std::unique_ptr<column>> cols;
  cols.reserve(nc);
  for (size_type k = 0; k < nc; ++k) {
    bool const with_mask = a.column(k).has_nulls() || b.column(k).has_nulls();
    auto const nk        = with_mask ? static_cast<size_type>(nulls[k]) : 0;
    cols.emplace_back(std::make_unique<column>(a.column(k).type(), n, std::move(data[k]),
                                               nk > 0 ? std::move(masks[k]) : rmm::device_buffer{0, stream, mr}, nk));
  }
  return std::make_unique<table>(std::move(cols));
}

}  // namespace

std::unique_ptr<table> merge(std::vector<table_view> const& tables_to_merge, std::vector<size_type> const& key_cols,
                             std::vector<order> const& column_order, std::vector<null_order> const& null_precedence,
                             rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  if (tables_to_merge.empty()) return std::make_unique<table>();
  auto const& first = tables_to_merge.front();
  CUDF_EXPECTS(!key_cols.empty(), "Empty key_cols");
  CUDF_EXPECTS(key_cols.size() <= static_cast<std::size_t>(first.num_columns()), "Too many values in key_cols");
  CUDF_EXPECTS(key_cols.size() == column_order.size(), "Mismatched size between key_cols and column_order");
  CUDF_EXPECTS(null_precedence.empty() || null_precedence.size() == key_cols.size(), "Mismatched size between key_cols and null_precedence");
  for (auto const& t : tables_to_merge) CUDF_EXPECTS(detail::same_types(first, t), "Mismatched column types");
  auto const keys = first.select(key_cols);  // std::out_of_range for an invalid index
  CUDF_EXPECTS(keys.num_columns() <= detail::MAX_KEYS, "merge: at most 32 key columns", std::invalid_argument);
  for (auto const& c : keys) detail::gx_type(c.type());  // cudf::data_type_error for a key that is no fixed-width numeric
  std::size_t total = 0;
  for (auto const& t : tables_to_merge) total += static_cast<std::size_t>(t.num_rows());
  CUDF_EXPECTS(total <= static_cast<std::size_t>(std::numeric_limits<size_type>::max()), "Total number of merged rows exceeds the column size limit",
               std::overflow_error);

  // the tables with rows, in the order given: a table without rows adds nothing, the others keep their place in the tie order
  struct run {
    table_view view;
    std::unique_ptr<table> owned;  // an intermediate result; empty for an input
  };
  std::vector<run> level;
  for (auto const& t : tables_to_merge)
    if (t.num_rows() > 0) level.push_back(run{t, nullptr});
  if (level.empty()) return detail::empty_like_table(first);
  if (level.size() == 1) return std::make_unique<table>(level.front().view, stream, mr);
  // a balanced tree over neighbours: a run is merged only with the run next to it, so equivalent rows never change sides
  while (level.size() > 1) {
    std::vector<run> next;
    for (std::size_t i = 0; i + 1 < level.size(); i += 2) {
      auto merged   = merge_two(level[i].view, level[i + 1].view, key_cols, column_order, null_precedence, stream, mr);
      auto const mv = merged->view();
      next.push_back(run{mv, std::move(merged)});
    }
    if (level.size() % 2) next.push_back(std::move(level.back()));  // the odd one out sits this level out
    level = std::move(next);
  }
  return std::move(level.front().owned);  // two or more runs: the last step was a merge
}

}  // namespace cudf
