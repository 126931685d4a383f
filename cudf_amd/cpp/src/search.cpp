// cudf::lower_bound / upper_bound over the C ABI (gx_search_bounds; cudf_amd/csrc/gx_merge.hip).
// reference: cpp/include/cudf/search.hpp, cpp/src/search/search_ordered.cu -- there thrust::lower_bound / upper_bound over row indices
// under the lexicographic row comparator; here one binary search per needle with the same comparator.  Stream-ordered, nothing is
// read back.
#include "common.hpp"
#include "ordered_rows.hpp"

#include <cudf/column/column_factories.hpp>
#include <cudf/search.hpp>

#include <stdexcept>

namespace cudf {
namespace {

std::unique_ptr<column> search_ordered(table_view const& haystack, table_view const& needles, std::vector<order> const& column_order,
                                       std::vector<null_order> const& null_precedence, bool upper, rmm::cuda_stream_view stream,
                                       rmm::device_async_resource_ref mr)
{
  CUDF_EXPECTS(detail::same_types(haystack, needles), "Mismatch between the columns of haystack and needles");
  CUDF_EXPECTS(column_order.size() == static_cast<std::size_t>(haystack.num_columns()), "Mismatch between number of columns and column order.");
  CUDF_EXPECTS(null_precedence.empty() || null_precedence.size() == static_cast<std::size_t>(haystack.num_columns()),
               "Mismatch between number of columns and null_precedence size.");
  CUDF_EXPECTS(haystack.num_columns() <= detail::MAX_KEYS, "search: at most 32 columns", std::invalid_argument);
  auto const n = needles.num_rows();
  if (n == 0 || haystack.num_columns() == 0) return make_empty_column(data_type{type_id::INT32});
  detail::key_order const ko{haystack, column_order, null_precedence};
  detail::key_side const h{haystack}, x{needles};
  rmm::device_buffer out{static_cast<std::size_t>(n) * sizeof(int32_t), stream, mr};
  detail::gx_check(gx_search_bounds(static_cast<int>(ko.dtypes.size()), ko.dtypes.data(), h.data.data(), h.valid.data(), h.begin.data(), h.rows,
                                    x.data.data(), x.valid.data(), x.begin.data(), x.rows, ko.descending.data(), ko.null_before.data(),
                                    upper ? 1 : 0, static_cast<int32_t*>(out.data()), detail::gxs(stream)),
                   upper ? "upper_bound" : "lower_bound");
  return std::make_unique<column>(data_type{type_id::INT32}, n, std::move(out), rmm::device_buffer{0, stream, mr}, 0);
}

}  // namespace

std::unique_ptr<column> lower_bound(table_view const& haystack, table_view const& needles, std::vector<order> const& column_order,
                                    std::vector<null_order> const& null_precedence, rmm::cuda_stream_view stream,
                                    rmm::device_async_resource_ref mr)
{
  return search_ordered(haystack, needles, column_order, null_precedence, false, stream, mr);
}

std::unique_ptr<column> upper_bound(table_view const& haystack, table_view const& needles, std::vector<order> const& column_order,
                                    std::vector<null_order> const& null_precedence, rmm::cuda_stream_view stream,
                                    rmm::device_async_resource_ref mr)
{
  return search_ordered(haystack, needles, column_order, null_precedence, true, stream, mr);
}

}  // namespace cudf
