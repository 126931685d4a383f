// cudf/replace.hpp -- null and value replacement (reference: cpp/include/cudf/replace.hpp; cpp/src/replace/nulls.cu, nans.cu,
// clamp.cu, replace.cu).  Kernels: cudf_amd/csrc/gx_replace.hip.  Fixed-width numeric and BOOL8 columns; strings, dictionaries
// and fixed-point are not built.  Common to every function below:
//   * a type mismatch between the input and a replacement, a bound or a list throws cudf::data_type_error;
//   * a sliced view (cudf::slice) is read in place, through its offset and the begin bit of its bitmap;
//   * an empty input gives an empty column of the input's type;
//   * the result carries a bitmap only if it holds a null; its null count is counted on the device and read once;
//   * where the call cannot change a row -- an input without nulls, an invalid replacement scalar, two invalid bounds, an empty
//     list -- the result is a copy of the input and nothing but that copy is launched.
#pragma once
#include <cudf/column/column.hpp>
#include <cudf/column/column_view.hpp>
#include <cudf/scalar/scalar.hpp>

#include <memory>

namespace cudf {

// which neighbouring valid value replaces a null
enum class replace_policy : bool { PRECEDING, FOLLOWING };

// out[i] = input[i] where it is valid, else replacement[i]; the row is null where both are.
// std::invalid_argument: the sizes differ.
std::unique_ptr<column> replace_nulls(column_view const& input, column_view const& replacement,
                                      rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                      rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());
// out[i] = input[i] where it is valid, else the scalar.  An invalid scalar replaces nothing.
std::unique_ptr<column> replace_nulls(column_view const& input, scalar const& replacement,
                                      rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                      rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());
// a null row takes the nearest valid value before (PRECEDING) or after (FOLLOWING) it; rows without one stay null.
std::unique_ptr<column> replace_nulls(column_view const& input, replace_policy const& policy,
                                      rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                      rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

// a valid NaN row takes replacement[i], value and validity; every other row, a null row included, is kept.
// std::invalid_argument: the input is not a float column, or the sizes differ.
std::unique_ptr<column> replace_nans(column_view const& input, column_view const& replacement,
                                     rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                     rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());
std::unique_ptr<column> replace_nans(column_view const& input, scalar const& replacement,
                                     rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                     rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

// out[i] = replacement_values[j] for the first j with input[i] == values_to_replace[j], else input[i].  == is the type's: NaN
// matches nothing, -0.0 matches +0.0.  A null input row stays null; a replaced row takes the validity of its replacement.
// The cost is rows x list length comparisons, as in the reference: meant for short lists.
// std::invalid_argument: the two lists differ in size, or values_to_replace has nulls.
std::unique_ptr<column> find_and_replace_all(column_view const& input, column_view const& values_to_replace,
                                             column_view const& replacement_values,
                                             rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                             rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

// out[i] = input[i] < lo ? lo_replace : (input[i] > hi ? hi_replace : input[i]) in the column's own type; an invalid bound does
// not bound, a NaN passes through; validity and null count are the input's.
// std::invalid_argument: lo_replace (hi_replace) is invalid while lo (hi) is valid.
std::unique_ptr<column> clamp(column_view const& input, scalar const& lo, scalar const& lo_replace, scalar const& hi,
                              scalar const& hi_replace, rmm::cuda_stream_view stream = cudf::get_default_stream(),
                              rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());
// the same with lo_replace = lo and hi_replace = hi
std::unique_ptr<column> clamp(column_view const& input, scalar const& lo, scalar const& hi,
                              rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                              rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

// every NaN becomes the positive quiet NaN, -0.0 becomes +0.0, everything else is copied bit for bit; validity is the input's.
// std::invalid_argument: the input is not a float column.
std::unique_ptr<column> normalize_nans_and_zeros(column_view const& input, rmm::cuda_stream_view stream = cudf::get_default_stream(),
                                                 rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());
// ... in place
void normalize_nans_and_zeros(mutable_column_view& in_out, rmm::cuda_stream_view stream = cudf::get_default_stream());

}  // namespace cudf
