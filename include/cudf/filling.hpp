// cudf/filling.hpp -- fill, repeat and sequence (reference: cpp/include/cudf/filling.hpp; cpp/src/filling/fill.cu, repeat.cu,
// sequence.cu).  Kernels: cudf_amd/csrc/gx_reshape.hip (gx_fill_range, gx_repeat_each, gx_repeat_map, gx_sequence).  Fixed-width
// numeric and BOOL8 columns; strings, lists, dictionaries and fixed-point are not built.  Common to every function below:
//   * a sliced view (cudf::slice) is read in place, through its offset and the begin bit of its bitmap;
//   * an empty input gives an empty result of the input's type(s);
//   * the result carries a bitmap only if it holds a null.
#pragma once
#include <cudf/column/column.hpp>
#include <cudf/column/column_view.hpp>
#include <cudf/scalar/scalar.hpp>
#include <cudf/table/table.hpp>
#include <cudf/table/table_view.hpp>

#include <memory>

namespace cudf {

// destination[begin, end) = value, in place.  An invalid scalar clears the range's validity bits, a valid one sets them (where
// the column has a bitmap); the column's null count is brought up to date.  begin == end does nothing.
// std::out_of_range: begin < 0, end > size or begin > end; cudf::data_type_error: the scalar's type is not the column's;
// std::invalid_argument: an invalid scalar and a column without a bitmap.
void fill_in_place(mutable_column_view& destination, size_type begin, size_type end, scalar const& value,
                   rmm::cuda_stream_view stream = cudf::get_default_stream());

// a copy of input with rows [begin, end) set to value.  With an invalid scalar the result has nulls in the range; with a valid one the
// range is valid and the other rows keep the input's validity.  begin == end is a copy, and nothing but the copy is launched.
// Throws as fill_in_place does (an invalid scalar is always accepted).
std::unique_ptr<column> fill(column_view const& input, size_type begin, size_type end, scalar const& value,
                             rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                             rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

// row i of every column repeated count[i] times.  The counts are cast to int64 and scanned on the device; the total is read once (it
// sizes the result), one expansion map is computed for the whole table and every column is gathered through it.  Negative entries
// in count are undefined behaviour, as in the reference.
// std::invalid_argument: count is not an integral column, has nulls, or differs in length from the table; std::overflow_error: the
// row total does not fit size_type.
std::unique_ptr<table> repeat(table_view const& input, column_view const& count, rmm::cuda_stream_view stream = cudf::get_default_stream(),
                              rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());
// every row repeated count times: one streaming launch per column, validity and null count included.
// std::invalid_argument: count < 0; std::overflow_error: num_rows x count does not fit size_type.
std::unique_ptr<table> repeat(table_view const& input, size_type count, rmm::cuda_stream_view stream = cudf::get_default_stream(),
                              rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

// out[i] = init + i * step in the scalars' type, a numeric type other than BOOL8.  Integers wrap modulo 2^w; floats round the product
// T(i) * step and then the sum (two roundings, no fused multiply-add).  The result has no nulls.
// std::invalid_argument: size < 0, an invalid init or step, a type that is not numeric or is BOOL8; cudf::data_type_error: init and
// step differ in type.
std::unique_ptr<column> sequence(size_type size, scalar const& init, scalar const& step,
                                 rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                 rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());
// the same with step 1
std::unique_ptr<column> sequence(size_type size, scalar const& init, rmm::cuda_stream_view stream = cudf::get_default_stream(),
                                 rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

}  // namespace cudf
