// cudf::binary_operation over the C ABI (gx_binary_op; cudf_amd/csrc/gx_elementwise.hip).
// reference: cpp/include/cudf/binaryop.hpp, cpp/src/binaryop/binaryop.cpp (the three overloads, the output mask as the AND of
// the operands' masks, the NULL_* operators writing their own), compiled/binary_ops.cuh.  Here one launch writes values, validity
// words and the null count; the operands and the result mask follow the models of DESIGN.md 3.6 (result_column.hpp).
#include "result_column.hpp"

#include <cudf/binaryop.hpp>

namespace cudf {
namespace {

using detail::source;

void check_operator(binary_operator op, source const& lhs, source const& rhs, data_type output_type)
{
  auto const out = detail::gx_type(output_type);
  // an operator this library does not build, whatever the types: INT32 operands are taken by every operator that is built
  CUDF_EXPECTS(gx_binary_op_supported(static_cast<int>(op), GX_INT32, GX_INT32, GX_INT32) == 1, "This binary operator is not built");
  CUDF_EXPECTS(gx_binary_op_supported(static_cast<int>(op), lhs.dtype(), rhs.dtype(), out) == 1,
               "Unsupported operator for these types", cudf::data_type_error);
}

std::unique_ptr<column> run(source const& lhs, source const& rhs, size_type n, binary_operator op, data_type output_type,
                            rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  if (n == 0) return make_empty_column(output_type);
  detail::result_column out{output_type, n, lhs.may_be_null || rhs.may_be_null, mask_state::UNINITIALIZED, stream, mr};
  detail::gx_check(gx_binary_op(static_cast<int>(op), lhs.dtype(), lhs.data, lhs.valid, lhs.begin_bit, lhs.scalar_valid, lhs.is_scalar,
                                rhs.dtype(), rhs.data, rhs.valid, rhs.begin_bit, rhs.scalar_valid, rhs.is_scalar, n,
                                static_cast<int>(output_type.id()), out.data(), out.valid(), out.nulls_dev(), detail::gxs(stream)),
                   "gx_binary_op");
  return out.finish();
}

}  // namespace

std::unique_ptr<column> binary_operation(column_view const& lhs, column_view const& rhs, binary_operator op, data_type output_type,
                                         rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  CUDF_EXPECTS(lhs.size() == rhs.size(), "Column sizes don't match");
  auto const l = detail::source_of(lhs), r = detail::source_of(rhs);
  check_operator(op, l, r, output_type);
  return run(l, r, lhs.size(), op, output_type, stream, mr);
}

std::unique_ptr<column> binary_operation(column_view const& lhs, scalar const& rhs, binary_operator op, data_type output_type,
                                         rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  auto const l = detail::source_of(lhs);
  auto r       = detail::source_of(rhs);
  check_operator(op, l, r, output_type);
  r.may_be_null = detail::scalar_may_be_null(rhs, lhs.size() > 0, stream);
  return run(l, r, lhs.size(), op, output_type, stream, mr);
}

std::unique_ptr<column> binary_operation(scalar const& lhs, column_view const& rhs, binary_operator op, data_type output_type,
                                         rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  auto l       = detail::source_of(lhs);
  auto const r = detail::source_of(rhs);
  check_operator(op, l, r, output_type);
  l.may_be_null = detail::scalar_may_be_null(lhs, rhs.size() > 0, stream);
  return run(l, r, rhs.size(), op, output_type, stream, mr);
}

namespace binops {
bool is_supported_operation(data_type out, data_type lhs, data_type rhs, binary_operator op)
{
  return gx_binary_op_supported(static_cast<int>(op), static_cast<int>(lhs.id()), static_cast<int>(rhs.id()), static_cast<int>(out.id())) == 1;
}
}  // namespace binops

}  // namespace cudf
