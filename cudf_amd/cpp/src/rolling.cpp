// cudf::rolling_window / grouped_rolling_window over the C ABI (gx_rolling_window; cudf_amd/csrc/gx_rolling.hip).
// reference: cpp/include/cudf/rolling.hpp, rolling.cu, grouped_rolling.cu -- there one thread per row loops over its window.  Here
// fixed windows take a tile kernel with two segmented scans in LDS (constant work per row), the rest a row loop; the groups of
// grouped_rolling_window are the runs of equal key rows: gx_group_heads per key column, then gx_group_offsets.
// Stream-ordered up to the read of the null count, which decides whether the result keeps its mask.
#include "result_column.hpp"

#include <cudf/rolling.hpp>

#include <algorithm>
#include <vector>

namespace cudf {
namespace {

struct plan {
  int op;
  data_type out_type;
};

plan plan_of(column_view const& input, size_type min_periods, rolling_aggregation const& agg)
{
  CUDF_EXPECTS(min_periods >= 0, "min_periods must be non-negative");
  auto const id = input.type().id();
  CUDF_EXPECTS(detail::is_gx_type(input.type()), "rolling_window: the input must be a fixed-width numeric or BOOL8 column");
  switch (agg.kind) {
    case aggregation::SUM: return {GX_OP_SUM, is_floating_point(input.type()) ? input.type() : data_type{id == type_id::UINT64 ? type_id::UINT64 : type_id::INT64}};
    case aggregation::MIN: return {GX_OP_MIN, input.type()};
    case aggregation::MAX: return {GX_OP_MAX, input.type()};
    case aggregation::MEAN: return {GX_OP_MEAN, data_type{type_id::FLOAT64}};
    case aggregation::COUNT_VALID: return {GX_OP_COUNT_VALID, data_type{type_id::INT32}};
    case aggregation::COUNT_ALL: return {GX_OP_COUNT_ALL, data_type{type_id::INT32}};
    default: CUDF_FAIL("rolling_window: only SUM, MIN, MAX, MEAN, COUNT_VALID and COUNT_ALL are provided");
  }
}

std::unique_ptr<column> run(column_view const& input, plan const& pl, int64_t preceding, int64_t following, int32_t const* pcol,
                            int32_t const* fcol, int32_t const* labels, int32_t const* offsets, size_type min_periods,
                            rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  auto const n = input.size();
  if (n == 0) return make_empty_column(pl.out_type);
  detail::result_column out{pl.out_type, n, true, mask_state::ALL_NULL, stream, mr};  // any window can fall short of min_periods
  detail::gx_check(gx_rolling_window(detail::gx_type(input.type()), detail::row0(input), input.has_nulls() ? input.null_mask() : nullptr,
                                     input.offset(), n, preceding, following, pcol, fcol, labels, offsets, min_periods, pl.op, out.data(),
                                     out.valid(), out.nulls_dev(), detail::gxs(stream)),
                   "gx_rolling_window");
  return out.finish();
}

}  // namespace

std::unique_ptr<column> rolling_window(column_view const& input, size_type preceding_window, size_type following_window, size_type min_periods,
                                       rolling_aggregation const& agg, rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  auto const pl = plan_of(input, min_periods, agg);
  return run(input, pl, preceding_window, following_window, nullptr, nullptr, nullptr, nullptr, min_periods, stream, mr);
}

std::unique_ptr<column> rolling_window(column_view const& input, column_view const& preceding_window, column_view const& following_window,
                                       size_type min_periods, rolling_aggregation const& agg, rmm::cuda_stream_view stream,
                                       rmm::device_async_resource_ref mr)
{
  auto const pl = plan_of(input, min_periods, agg);
  for (auto const* w : {&preceding_window, &following_window}) {
    CUDF_EXPECTS(w->type().id() == type_id::INT32, "rolling_window: window columns must be INT32");
    CUDF_EXPECTS(!w->nullable(), "rolling_window: window columns must not be nullable");
    CUDF_EXPECTS(w->size() == input.size(), "rolling_window: window columns must have one row per input row");
  }
  return run(input, pl, 0, 0, static_cast<int32_t const*>(detail::row0(preceding_window)), static_cast<int32_t const*>(detail::row0(following_window)),
             nullptr, nullptr, min_periods, stream, mr);
}

std::unique_ptr<column> grouped_rolling_window(table_view const& group_keys, column_view const& input, size_type preceding_window,
                                               size_type following_window, size_type min_periods, rolling_aggregation const& agg,
                                               rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  if (group_keys.num_columns() == 0) return rolling_window(input, preceding_window, following_window, min_periods, agg, stream, mr);
  auto const pl = plan_of(input, min_periods, agg);
  CUDF_EXPECTS(group_keys.num_rows() == input.size(), "grouped_rolling_window: the keys must have one row per input row");
  for (auto const& c : group_keys) detail::gx_type(c.type());
  auto const n = input.size();
  if (n == 0) return make_empty_column(pl.out_type);
  // rows differ when ANY key column differs: one pass per column, ORed into the head flags
  rmm::device_buffer heads{static_cast<std::size_t>(n), stream};
  rmm::device_uvector<int32_t> labels(static_cast<std::size_t>(n), stream), offsets(static_cast<std::size_t>(n) + 1, stream);
  std::vector<rmm::device_buffer> holders(static_cast<std::size_t>(group_keys.num_columns()));
  for (size_type k = 0; k < group_keys.num_columns(); ++k) {
    auto const& c    = group_keys.column(k);
    auto const* mask = c.has_nulls() ? detail::rebased_mask(c, holders[k], stream) : nullptr;
    detail::gx_check(gx_group_heads(detail::gx_type(c.type()), detail::row0(c), mask, nullptr, n, k > 0 ? 1 : 0,
                                    static_cast<uint8_t*>(heads.data()), detail::gxs(stream)),
                     "rolling group heads");
  }
  rmm::device_buffer ng{sizeof(int64_t), stream};
  auto scratch = detail::run_with_scratch(
    [&](void* t, std::size_t* b) {
      return gx_group_offsets(static_cast<uint8_t const*>(heads.data()), n, labels.data(), offsets.data(), nullptr,
                              static_cast<int64_t*>(ng.data()), t, b, detail::gxs(stream));
    },
    "rolling group offsets", stream);
  return run(input, pl, preceding_window, following_window, nullptr, nullptr, labels.data(), offsets.data(), min_periods, stream, mr);
}

}  // namespace cudf
