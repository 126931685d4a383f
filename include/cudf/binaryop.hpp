// cudf/binaryop.hpp -- element-wise binary operations between two columns, or a column and a scalar (reference:
// cpp/include/cudf/binaryop.hpp; cpp/src/binaryop/binaryop.cpp, compiled/binary_ops.cuh, compiled/operation.cuh).
// One kernel file (cudf_amd/csrc/gx_elementwise.hip) covers the type x type x type x operator space: the operands are converted to
// the type the usual arithmetic conversions give for them, the operator runs there, and the result is cast to output_type
// (include/cudf_amd/gx.h, gx_binary_op, states the value of every operator).
#pragma once
#include <cudf/column/column.hpp>
#include <cudf/column/column_view.hpp>
#include <cudf/scalar/scalar.hpp>

#include <cstdint>
#include <memory>

namespace cudf {

// the reference's enumerators in the reference's order, so that a caller's integer values mean the same
enum class binary_operator : int32_t {
  ADD,                   // operator +
  SUB,                   // operator -
  MUL,                   // operator *
  DIV,                   // operator / in the common type of lhs and rhs (integers truncate)
  TRUE_DIV,              // operator / after promoting both sides to double
  FLOOR_DIV,             // integers: exact floor division; floats: NumPy's floor_divide (floor(x / y) wherever that is exact)
  MOD,                   // operator % (sign of the dividend), fmod on floats
  PMOD,                  // positive modulo: ((x % y) + y) % y
  PYMOD,                 // operator % of Python: the sign of the divisor
  POW,                   // pow(double(x), double(y)); powf for float operands
  INT_POW,               // integer power by squaring, wrapping; a negative exponent gives 0
  LOG_BASE,              // not built: throws cudf::logic_error
  ATAN2,                 // not built: throws cudf::logic_error
  SHIFT_LEFT,            // operator <<
  SHIFT_RIGHT,           // operator >> (arithmetic on signed types)
  SHIFT_RIGHT_UNSIGNED,  // operator >>> of Java: lhs reinterpreted as the unsigned type of its own width
  BITWISE_AND,           // operator &
  BITWISE_OR,            // operator |
  BITWISE_XOR,           // operator ^
  LOGICAL_AND,           // operator &&
  LOGICAL_OR,            // operator ||
  EQUAL,                 // operator ==
  NOT_EQUAL,             // operator !=
  LESS,                  // operator <
  GREATER,               // operator >
  LESS_EQUAL,            // operator <=
  GREATER_EQUAL,         // operator >=
  NULL_EQUALS,           // true when both are null, false when one is, else ==; the result has no nulls
  NULL_NOT_EQUALS,       // the negation of NULL_EQUALS
  NULL_MAX,              // the maximum of the valid operands; null when both are null
  NULL_MIN,              // the minimum of the valid operands; null when both are null
  GENERIC_BINARY,        // not built (the reference compiles a PTX string): throws cudf::logic_error
  NULL_LOGICAL_AND,      // Kleene AND: a valid false decides the row, otherwise null when a side is null
  NULL_LOGICAL_OR,       // Kleene OR: a valid true decides the row, otherwise null when a side is null
  INVALID_BINARY         // the end of the list: throws cudf::logic_error
};

// out[i] = cast<output_type>(lhs[i] op rhs[i]).  A row is null where either operand is (the NULL_* operators have their own
// rules, above); the result has a null mask only if an operand has nulls (a column) or is invalid (a scalar).  Sliced views are
// read in place.  Empty operands give an empty column of output_type.
// cudf::logic_error: "Column sizes don't match" (lhs.size() != rhs.size()), an operator that is not built (LOG_BASE, ATAN2,
// GENERIC_BINARY); cudf::data_type_error: an operand or output_type is not a fixed-width numeric or BOOL8 type, or the operator
// does not take the operands (bitwise, shifts and INT_POW on floats).
std::unique_ptr<column> binary_operation(column_view const& lhs, column_view const& rhs, binary_operator op, data_type output_type,
                                         rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                         rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());
// a scalar stands for a column of equal rows; an invalid scalar makes every row null (except under the NULL_* operators)
std::unique_ptr<column> binary_operation(column_view const& lhs, scalar const& rhs, binary_operator op, data_type output_type,
                                         rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                         rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());
std::unique_ptr<column> binary_operation(scalar const& lhs, column_view const& rhs, binary_operator op, data_type output_type,
                                         rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                         rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

namespace binops {
// whether binary_operation takes this combination (host arithmetic: nothing is launched)
bool is_supported_operation(data_type out, data_type lhs, data_type rhs, binary_operator op);
}  // namespace binops

}  // namespace cudf
