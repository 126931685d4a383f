// cudf::unary_operation, cast, is_null / is_valid, is_nan / is_not_nan over the C ABI (gx_unary_op, gx_cast, gx_bitmask_to_bool8;
// cudf_amd/csrc/gx_elementwise.hip).  reference: cpp/include/cudf/unary.hpp, cpp/src/unary/math_ops.cu, cast_ops.cu, null_ops.cu,
// nan_ops.cu.  The kernels do not touch validity: the result takes a copy of the input's bits (re-based to bit 0 for a sliced
// view) and its null count, so nothing is read back.
#include "common.hpp"

#include <cudf/column/column_factories.hpp>
#include <cudf/null_mask.hpp>
#include <cudf/unary.hpp>

namespace cudf {
namespace {

std::unique_ptr<column> run_unary(column_view const& input, int op, data_type out_type, rmm::cuda_stream_view stream,
                                  rmm::device_async_resource_ref mr)
{
  auto const in  = detail::gx_type(input.type());
  auto const out = detail::gx_type(out_type);
  bool const built = op == GX_UNOP_SQRT || op == GX_UNOP_CEIL || op == GX_UNOP_FLOOR || op == GX_UNOP_ABS || op == GX_UNOP_RINT ||
                     op == GX_UNOP_BIT_INVERT || op == GX_UNOP_NOT || op == GX_UNOP_NEGATE || op == GX_UNOP_IS_NAN || op == GX_UNOP_IS_NOT_NAN;
  CUDF_EXPECTS(built, "This unary operator is not built");
  CUDF_EXPECTS(gx_unary_op_supported(op, in, out) == 1, "Unsupported unary operator for this type", cudf::data_type_error);
  auto const n = input.size();
  if (n == 0) return make_empty_column(out_type);
  rmm::device_buffer data{static_cast<std::size_t>(n) * size_of(out_type), stream, mr};
  detail::gx_check(gx_unary_op(op, in, detail::row0(input), n, out, data.data(), detail::gxs(stream)), "gx_unary_op");
  return std::make_unique<column>(out_type, n, std::move(data), detail::mask_of(input, stream, mr), input.null_count());
}

std::unique_ptr<column> validity_as_bool(column_view const& input, bool invert, rmm::cuda_stream_view stream,
                                         rmm::device_async_resource_ref mr)
{
  auto const n = input.size();
  if (n == 0) return make_empty_column(type_id::BOOL8);
  rmm::device_buffer data{static_cast<std::size_t>(n), stream, mr};
  detail::gx_check(gx_bitmask_to_bool8(input.has_nulls() ? input.null_mask() : nullptr, input.offset(), n, invert ? 1 : 0,
                                       static_cast<uint8_t*>(data.data()), detail::gxs(stream)),
                   "gx_bitmask_to_bool8");
  return std::make_unique<column>(data_type{type_id::BOOL8}, n, std::move(data), rmm::device_buffer{0, stream, mr}, 0);
}

}  // namespace

std::unique_ptr<column> unary_operation(column_view const& input, unary_operator op, rmm::cuda_stream_view stream,
                                        rmm::device_async_resource_ref mr)
{
  auto const out = op == unary_operator::NOT ? data_type{type_id::BOOL8} : input.type();
  return run_unary(input, static_cast<int>(op), out, stream, mr);
}

bool is_supported_cast(data_type from, data_type to) noexcept
{
  return detail::is_gx_type(from) && detail::is_gx_type(to);
}

std::unique_ptr<column> cast(column_view const& input, data_type out_type, rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  CUDF_EXPECTS(is_supported_cast(input.type(), out_type), "Column type must be numeric or BOOL8", cudf::data_type_error);
  auto const n = input.size();
  if (n == 0) return make_empty_column(out_type);
  rmm::device_buffer data{static_cast<std::size_t>(n) * size_of(out_type), stream, mr};
  detail::gx_check(gx_cast(static_cast<int>(input.type().id()), detail::row0(input), n, static_cast<int>(out_type.id()), data.data(),
                           detail::gxs(stream)),
                   "gx_cast");
  return std::make_unique<column>(out_type, n, std::move(data), detail::mask_of(input, stream, mr), input.null_count());
}

std::unique_ptr<column> is_null(column_view const& input, rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  return validity_as_bool(input, true, stream, mr);
}

std::unique_ptr<column> is_valid(column_view const& input, rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  return validity_as_bool(input, false, stream, mr);
}

std::unique_ptr<column> is_nan(column_view const& input, rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  return run_unary(input, GX_UNOP_IS_NAN, data_type{type_id::BOOL8}, stream, mr);
}

std::unique_ptr<column> is_not_nan(column_view const& input, rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  return run_unary(input, GX_UNOP_IS_NOT_NAN, data_type{type_id::BOOL8}, stream, mr);
}

}  // namespace cudf
