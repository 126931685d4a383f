// cudf/unary.hpp -- element-wise unary operations, casts and the null / NaN predicates (reference: cpp/include/cudf/unary.hpp;
// cpp/src/unary/math_ops.cu, cast_ops.cu, null_ops.cu, nan_ops.cu).  Kernels: cudf_amd/csrc/gx_elementwise.hip.
#pragma once
#include <cudf/column/column.hpp>
#include <cudf/column/column_view.hpp>

#include <cstdint>
#include <memory>

namespace cudf {

// the reference's enumerators in the reference's order.  Built: SQRT, CEIL, FLOOR, ABS, RINT, BIT_INVERT, NOT, NEGATE; the others
// throw cudf::logic_error.
enum class unary_operator : int32_t {
  SIN, COS, TAN, ARCSIN, ARCCOS, ARCTAN, SINH, COSH, TANH, ARCSINH, ARCCOSH, ARCTANH, EXP, LOG,
  SQRT,        // floats
  CBRT,
  CEIL,        // floats
  FLOOR,       // floats
  ABS,         // numeric types; the identity on unsigned
  RINT,        // floats; halves round to even
  BIT_COUNT,
  BIT_INVERT,  // integers, not BOOL8
  NOT,         // any type -> BOOL8: x == 0
  NEGATE       // numeric types; wraps on unsigned and at the minimum of a signed type
};

// out[i] = op(input[i]) in the input's type (NOT: BOOL8).  The result carries a copy of the input's validity and its null count.
// cudf::logic_error: an operator that is not built; cudf::data_type_error: the operator does not take the input's type.
std::unique_ptr<column> unary_operation(column_view const& input, unary_operator op,
                                        rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                        rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

// static_cast<out_type>(input[i]); a cast to BOOL8 is x != 0.  Validity and null count are the input's.
// cudf::data_type_error: is_supported_cast(input.type(), out_type) is false.
std::unique_ptr<column> cast(column_view const& input, data_type out_type, rmm::cuda_stream_view stream = cudf::get_default_stream(),
                             rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());
// both types fixed-width numeric or BOOL8
bool is_supported_cast(data_type from, data_type to) noexcept;

// BOOL8 columns without nulls: input[i] is null / is valid.  Any column type.
std::unique_ptr<column> is_null(column_view const& input, rmm::cuda_stream_view stream = cudf::get_default_stream(),
                                rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());
std::unique_ptr<column> is_valid(column_view const& input, rmm::cuda_stream_view stream = cudf::get_default_stream(),
                                 rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());
// BOOL8 columns with the input's validity: input[i] is / is not a NaN.  cudf::data_type_error: the input is not a float column.
std::unique_ptr<column> is_nan(column_view const& input, rmm::cuda_stream_view stream = cudf::get_default_stream(),
                               rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());
std::unique_ptr<column> is_not_nan(column_view const& input, rmm::cuda_stream_view stream = cudf::get_default_stream(),
                                   rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

}  // namespace cudf
