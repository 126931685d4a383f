// cudf/reshape.hpp -- interleave_columns and tile (reference: cpp/include/cudf/reshape.hpp; cpp/src/reshape/interleave_columns.cu,
// tile.cu).  Kernels: cudf_amd/csrc/gx_reshape.hip (gx_interleave, gx_tile).  Fixed-width numeric and BOOL8 columns; strings,
// lists, dictionaries and fixed-point are not built.  Common to both:
//   * a sliced view (cudf::slice) is read in place, through its offset and the begin bit of its bitmap;
//   * the result carries a bitmap only if it holds a null; its null count is counted on the device and read once.
#pragma once
#include <cudf/column/column.hpp>
#include <cudf/table/table.hpp>
#include <cudf/table/table_view.hpp>

#include <memory>

namespace cudf {

// one column: row 0 of every input column, then row 1, ...: out[i * num_columns + j] = input.column(j)[i].  A table without rows
// gives an empty column of the columns' type.
// std::invalid_argument: the table has no columns; cudf::data_type_error: the columns differ in type;
// std::overflow_error: num_rows x num_columns does not fit size_type.
std::unique_ptr<column> interleave_columns(table_view const& input, rmm::cuda_stream_view stream = cudf::get_default_stream(),
                                           rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

// the rows of the table laid down count times: out.column(k)[r * num_rows + i] = input.column(k)[i].  count == 0 or a table without
// rows gives empty columns of the input's types.
// std::invalid_argument: count < 0; std::overflow_error: num_rows x count does not fit size_type.
std::unique_ptr<table> tile(table_view const& input, size_type count, rmm::cuda_stream_view stream = cudf::get_default_stream(),
                            rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

}  // namespace cudf
