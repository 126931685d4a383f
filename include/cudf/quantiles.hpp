// cudf/quantiles.hpp -- cudf::quantile and cudf::quantiles (reference: cpp/include/cudf/quantiles.hpp; impl
// cpp/src/quantiles/quantile.cu, quantiles.cu).  The tdigest-based percentile_approx is not provided.
#pragma once
#include <cudf/column/column.hpp>
#include <cudf/column/column_view.hpp>
#include <cudf/table/table.hpp>
#include <cudf/table/table_view.hpp>
#include <cudf/types.hpp>
#include <cudf/utilities/default_stream.hpp>
#include <cudf/utilities/memory_resource.hpp>

#include <memory>
#include <vector>

namespace cudf {

// The values of `input` at the quantiles q, in the EXISTING order of the column or, with a non-empty ordered_indices (an INT32 map of
// input.size() rows), in the order it gives: this function does not sort.  For each q: pos = q * (size - 1) with q clamped to
// [0, 1], nulls counted as rows; LOWER / HIGHER / NEAREST (ties to even) take the row at floor / ceil / nearbyint(pos), LINEAR and
// MIDPOINT combine the rows at floor and ceil in double.  exact: a FLOAT64 column; !exact: the input's type (LINEAR / MIDPOINT: the
// double cast to it; otherwise the element itself).  A result is null when a row it reads is null.  An empty input gives q.size()
// nulls, an empty q an empty column.  At most 64 quantiles are looked up per kernel call; longer lists take several.
// cudf::data_type_error: input not numeric, or BOOL8.  std::invalid_argument: a non-empty ordered_indices that is not INT32, has
// nulls or has another row count than the input; a NaN quantile.
std::unique_ptr<column> quantile(column_view const& input, std::vector<double> const& q, interpolation interp = interpolation::LINEAR,
                                 column_view const& ordered_indices = {}, bool exact = true,
                                 rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                 rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

// Whole ROWS of `input` at the quantiles q of its lexicographic order: the existing sorted_order under column_order /
// null_precedence (one entry per column, or empty) unless is_input_sorted, then one gather at the lower / higher / nearest index of
// each q.  std::invalid_argument: LINEAR or MIDPOINT (the interpolation must be non-arithmetic), a table without rows, a NaN quantile.
std::unique_ptr<table> quantiles(table_view const& input, std::vector<double> const& q, interpolation interp = interpolation::NEAREST,
                                 cudf::sorted is_input_sorted = sorted::NO, std::vector<order> const& column_order = {},
                                 std::vector<null_order> const& null_precedence = {},
                                 rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                 rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

}  // namespace cudf
