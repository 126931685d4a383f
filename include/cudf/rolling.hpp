// cudf/rolling.hpp -- cudf::rolling_window and cudf::grouped_rolling_window: an aggregation over a window of rows around every row
// (reference: cpp/include/cudf/rolling.hpp; impl rolling.cu, grouped_rolling.cu, rolling_detail.cuh).
// Provided: fixed windows, one window per row, fixed windows inside groups; SUM, MIN, MAX, MEAN, COUNT_VALID, COUNT_ALL.
// Not provided: LEAD / LAG, VARIANCE / STD, ROW_NUMBER, COLLECT_LIST / COLLECT_SET, the default_outputs overload, range and time windows.
#pragma once
#include <cudf/aggregation.hpp>
#include <cudf/column/column.hpp>
#include <cudf/table/table_view.hpp>
#include <cudf/types.hpp>
#include <cudf/utilities/default_stream.hpp>
#include <cudf/utilities/memory_resource.hpp>

#include <memory>

namespace cudf {

// The window of row i is rows [i - preceding_window + 1, i + following_window] (preceding_window counts row i itself), cut to the
// column -- in grouped_rolling_window to the row's group.  Negative values are legal: such a window does not hold row i and may be
// empty.  input: a fixed-width numeric or BOOL8 column; sliced views work.
// Result, one row per input row: SUM of integers and BOOL8 -> INT64 (wrapping; UINT64 -> UINT64), SUM of floats -> the input type
// (FLOAT32 accumulated in double), MIN / MAX -> the input type (NaN greater than every number, -0.0 == +0.0), MEAN -> FLOAT64,
// COUNT_VALID / COUNT_ALL -> INT32.  The null mask is kept only when a row is null.
// Validity: SUM / MIN / MAX / MEAN -- a row is valid iff its window holds at least max(min_periods, 1) valid values: a window
// without a valid value is null, never an identity, also at min_periods == 0 (a deliberate choice; the reference's handling of
// min_periods == 0 is not copied).  COUNT_VALID / COUNT_ALL -- a row is valid iff its cut window has at least min_periods rows.
// Cost: constant per row for fixed windows of up to 2048 rows besides row i; O(window) per row beyond that and for per-row windows.
// cudf::logic_error: min_periods < 0, an aggregation other than the six, an input that is not numeric / BOOL8.
std::unique_ptr<column> rolling_window(column_view const& input, size_type preceding_window, size_type following_window,
                                       size_type min_periods, rolling_aggregation const& agg,
                                       rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                       rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

// One window per row: preceding_window / following_window are non-nullable INT32 columns of input.size() rows
// (cudf::logic_error otherwise).
std::unique_ptr<column> rolling_window(column_view const& input, column_view const& preceding_window,
                                       column_view const& following_window, size_type min_periods, rolling_aggregation const& agg,
                                       rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                       rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

// Groups are runs of equal rows of group_keys (fixed-width numeric columns, any mix of types, nulls equal to nulls); a window never
// leaves its row's group.  A key table without columns is the ungrouped call.  cudf::logic_error: group_keys.num_rows() !=
// input.size().
std::unique_ptr<column> grouped_rolling_window(table_view const& group_keys, column_view const& input, size_type preceding_window,
                                               size_type following_window, size_type min_periods, rolling_aggregation const& agg,
                                               rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                               rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

}  // namespace cudf
