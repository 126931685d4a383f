// cudf::binary_operation over the C ABI (gx_binary_op; cudf_amd/csrc/gx_elementwise.hip).
// reference: cpp/include/cudf/binaryop.hpp, cpp/src/binaryop/binaryop.cpp (the three overloads, the output mask as the AND of
// the operands' masks, the NULL_* operators writing their own), compiled/binary_ops.cuh.  Here one launch writes values, validity
// words and the null count; sliced views are read in place (offset data pointer, begin bit).  A mask is allocated only when an
// operand can be null, and kept only when a row is: the one host read of this path, as copy_if_else has it (copying.cpp).
#include "common.hpp"

#include <cudf/binaryop.hpp>
#include <cudf/column/column_factories.hpp>
#include <cudf/null_mask.hpp>

namespace cudf {
namespace {

struct operand {
  void const* data{nullptr};
  uint32_t const* valid{nullptr};
  int64_t begin_bit{0};
  uint8_t const* scalar_valid{nullptr};
  int is_scalar{0};
  bool may_be_null{false};
  int dtype{0};
};

operand operand_of(column_view const& c)
{
  operand o;
  o.dtype       = detail::gx_type(c.type());
  o.data        = detail::row0(c);
  o.valid       = c.has_nulls() ? c.null_mask() : nullptr;
  o.begin_bit   = c.offset();
  o.may_be_null = c.has_nulls();
  return o;
}

operand operand_of(scalar const& s)
{
  operand o;
  o.dtype = detail::gx_type(s.type());
  o.data  = s.device_value_ptr();
  CUDF_EXPECTS(o.data != nullptr, "Only fixed-width scalars are supported on this path", cudf::data_type_error);
  o.scalar_valid = reinterpret_cast<uint8_t const*>(s.validity_data());
  o.is_scalar    = 1;
  return o;
}

void check_operator(binary_operator op, operand const& lhs, operand const& rhs, data_type output_type)
{
  auto const out = detail::gx_type(output_type);
  // an operator this library does not build, whatever the types: INT32 operands are taken by every operator that is built
  CUDF_EXPECTS(gx_binary_op_supported(static_cast<int>(op), GX_INT32, GX_INT32, GX_INT32) == 1, "This binary operator is not built");
  CUDF_EXPECTS(gx_binary_op_supported(static_cast<int>(op), lhs.dtype, rhs.dtype, out) == 1,
               "Unsupported operator for these types", cudf::data_type_error);
}

std::unique_ptr<column> run(operand const& lhs, operand const& rhs, size_type n, binary_operator op, data_type output_type,
                            rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  if (n == 0) return make_empty_column(output_type);
  rmm::device_buffer data{static_cast<std::size_t>(n) * size_of(output_type), stream, mr};
  bool const with_mask = lhs.may_be_null || rhs.may_be_null;
  auto mask            = create_null_mask(n, with_mask ? mask_state::UNINITIALIZED : mask_state::UNALLOCATED, stream, mr);
  rmm::device_buffer nulls_dev{sizeof(int64_t), stream};
  detail::gx_check(gx_binary_op(static_cast<int>(op), lhs.dtype, lhs.data, lhs.valid, lhs.begin_bit, lhs.scalar_valid, lhs.is_scalar,
                                rhs.dtype, rhs.data, rhs.valid, rhs.begin_bit, rhs.scalar_valid, rhs.is_scalar, n,
                                static_cast<int>(output_type.id()), data.data(), with_mask ? static_cast<uint32_t*>(mask.data()) : nullptr,
                                with_mask ? static_cast<int64_t*>(nulls_dev.data()) : nullptr, detail::gxs(stream)),
                   "gx_binary_op");
  auto const nulls = with_mask ? static_cast<size_type>(detail::read_i64(static_cast<int64_t const*>(nulls_dev.data()), stream)) : 0;
  return std::make_unique<column>(output_type, n, std::move(data), nulls > 0 ? std::move(mask) : rmm::device_buffer{0, stream, mr}, nulls);
}

}  // namespace

std::unique_ptr<column> binary_operation(column_view const& lhs, column_view const& rhs, binary_operator op, data_type output_type,
                                         rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  CUDF_EXPECTS(lhs.size() == rhs.size(), "Column sizes don't match");
  auto const l = operand_of(lhs), r = operand_of(rhs);
  check_operator(op, l, r, output_type);
  return run(l, r, lhs.size(), op, output_type, stream, mr);
}

std::unique_ptr<column> binary_operation(column_view const& lhs, scalar const& rhs, binary_operator op, data_type output_type,
                                         rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  auto const l = operand_of(lhs);
  auto r       = operand_of(rhs);
  check_operator(op, l, r, output_type);
  r.may_be_null = lhs.size() > 0 && !rhs.is_valid(stream);
  return run(l, r, lhs.size(), op, output_type, stream, mr);
}

std::unique_ptr<column> binary_operation(scalar const& lhs, column_view const& rhs, binary_operator op, data_type output_type,
                                         rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  auto l       = operand_of(lhs);
  auto const r = operand_of(rhs);
  check_operator(op, l, r, output_type);
  l.may_be_null = rhs.size() > 0 && !lhs.is_valid(stream);
  return run(l, r, rhs.size(), op, output_type, stream, mr);
}

namespace binops {
bool is_supported_operation(data_type out, data_type lhs, data_type rhs, binary_operator op)
{
  return gx_binary_op_supported(static_cast<int>(op), static_cast<int>(lhs.id()), static_cast<int>(rhs.id()), static_cast<int>(out.id())) == 1;
}
}  // namespace binops

}  // namespace cudf
