// cudf/transpose.hpp -- a table turned on its side (reference: cpp/include/cudf/transpose.hpp; cpp/src/transpose/transpose.cu, which
// interleaves the columns and slices the result).  Kernel: gx_interleave (cudf_amd/csrc/gx_reshape.hip).  Fixed-width numeric and
// BOOL8 columns; strings, lists, dictionaries and fixed-point are not built.
#pragma once
#include <cudf/column/column.hpp>
#include <cudf/table/table_view.hpp>

#include <memory>
#include <utility>

namespace cudf {

// The column owns the data: the interleave of the input.  The view is num_rows columns of num_columns rows each, sliced out of that
// column: view.column(i)[j] = input.column(j)[i].  If one input column has nulls the column carries a bitmap and every view
// column its own null count (counted on the device, read once for all of them).  Sliced input views are read in place.  A table
// without columns or without rows gives an empty column and an empty view.
// cudf::data_type_error: the columns differ in type; std::overflow_error: num_rows x num_columns does not fit size_type.
std::pair<std::unique_ptr<column>, table_view> transpose(table_view const& input, rmm::cuda_stream_view stream = cudf::get_default_stream(),
                                                         rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

}  // namespace cudf
