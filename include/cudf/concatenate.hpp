// cudf/concatenate.hpp -- cudf::concatenate of columns and of tables, cudf::concatenate_masks
// (reference: cpp/include/cudf/concatenate.hpp; impl cpp/src/copying/concatenate.cu).
#pragma once
#include <cudf/column/column.hpp>
#include <cudf/table/table.hpp>
#include <cudf/table/table_view.hpp>
#include <cudf/utilities/default_stream.hpp>
#include <cudf/utilities/memory_resource.hpp>
#include <cudf/utilities/span.hpp>
#include <rmm/device_buffer.hpp>

#include <memory>

namespace cudf {

// The rows of columns_to_concat[0], then of [1], ...: one fused launch for data, validity and any number of inputs (fixed-width
// columns; sliced views work).  The result has a null mask only if an input has nulls; its null count is the sum of the views'
// null counts, so nothing is read back and the call stays stream-ordered.  One input gives a copy, inputs without rows an empty
// column of the type.
// std::invalid_argument: an empty span; cudf::data_type_error: the types differ; std::overflow_error: more rows in all than
// size_type holds (decided before any device call).
std::unique_ptr<column> concatenate(host_span<column_view const> columns_to_concat,
                                    rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                    rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

// Column by column.  cudf::logic_error: the tables differ in their number of columns; the throws above otherwise.
std::unique_ptr<table> concatenate(host_span<table_view const> tables_to_concat,
                                   rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                   rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

// The validity bitmap of the concatenation alone: bit i is set iff row i of the concatenation is valid (views without a mask
// contribute set bits).  An empty buffer when no view is nullable.
rmm::device_buffer concatenate_masks(host_span<column_view const> views, rmm::cuda_stream_view stream = cudf::get_default_stream(),
                                     rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

}  // namespace cudf
