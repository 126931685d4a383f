// cudf::replace_nulls, replace_nans, find_and_replace_all, clamp and normalize_nans_and_zeros over the C ABI (gx_replace_nulls,
// gx_replace_nulls_policy, gx_replace_nans, gx_find_and_replace, gx_clamp, gx_normalize_nans_and_zeros;
// cudf_amd/csrc/gx_replace.hip).  reference: cpp/include/cudf/replace.hpp, cpp/src/replace/nulls.cu, nans.cu, replace.cu, clamp.cu.
// One launch writes values, validity words and the null count; replacements and the result mask follow the models of DESIGN.md 3.6
// (result_column.hpp).  A call that cannot change a row returns a copy of its input.
#include "result_column.hpp"

#include <cudf/replace.hpp>

#include <stdexcept>

namespace cudf {
namespace {

using detail::scalar_device_value;

// a copy of the input's rows; as every result here it has a mask only when a row is null
std::unique_ptr<column> copy_of(column_view const& input, rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  if (input.has_nulls()) return std::make_unique<column>(input, stream, mr);
  return std::make_unique<column>(column_view{input.type(), input.size(), input.head<void>(), nullptr, 0, input.offset()}, stream, mr);
}

// `r`: the replacement column, or a scalar the caller has found VALID (its validity byte is not handed to the kernel)
std::unique_ptr<column> run_replace(bool nans, column_view const& input, detail::source const& r, rmm::cuda_stream_view stream,
                                    rmm::device_async_resource_ref mr)
{
  auto const n = input.size();
  // replace_nulls: a row is null where both sides are; replace_nans: where the input is, or a NaN row's replacement is
  bool const with_mask = nans ? (input.has_nulls() || r.valid != nullptr) : (input.has_nulls() && r.valid != nullptr);
  detail::result_column out{input.type(), n, with_mask, mask_state::UNINITIALIZED, stream, mr};
  auto const* ival = input.has_nulls() ? input.null_mask() : nullptr;
  if (nans)
    detail::gx_check(gx_replace_nans(detail::gx_type(input.type()), detail::row0(input), ival, input.offset(), r.data, r.valid, r.begin_bit,
                                     nullptr, r.is_scalar, n, out.data(), out.valid(), out.nulls_dev(), detail::gxs(stream)),
                     "gx_replace_nans");
  else
    detail::gx_check(gx_replace_nulls(static_cast<int>(size_of(input.type())), detail::row0(input), ival, input.offset(), r.data, r.valid,
                                      r.begin_bit, nullptr, r.is_scalar, n, out.data(), out.valid(), out.nulls_dev(), detail::gxs(stream)),
                     "gx_replace_nulls");
  return out.finish();
}

}  // namespace

std::unique_ptr<column> replace_nulls(column_view const& input, column_view const& replacement, rmm::cuda_stream_view stream,
                                      rmm::device_async_resource_ref mr)
{
  (void)detail::gx_type(input.type());
  CUDF_EXPECTS(input.type() == replacement.type(), "Data type mismatch", cudf::data_type_error);
  CUDF_EXPECTS(input.size() == replacement.size(), "Column size mismatch", std::invalid_argument);
  if (input.size() == 0) return make_empty_column(input.type());
  if (!input.has_nulls()) return copy_of(input, stream, mr);
  return run_replace(false, input, detail::source_of(replacement), stream, mr);
}

std::unique_ptr<column> replace_nulls(column_view const& input, scalar const& replacement, rmm::cuda_stream_view stream,
                                      rmm::device_async_resource_ref mr)
{
  (void)detail::gx_type(input.type());
  CUDF_EXPECTS(input.type() == replacement.type(), "Data type mismatch", cudf::data_type_error);
  if (input.size() == 0) return make_empty_column(input.type());
  auto const r = detail::source_of(replacement);
  if (!input.has_nulls() || !replacement.is_valid(stream)) return copy_of(input, stream, mr);
  return run_replace(false, input, r, stream, mr);
}

std::unique_ptr<column> replace_nulls(column_view const& input, replace_policy const& policy, rmm::cuda_stream_view stream,
                                      rmm::device_async_resource_ref mr)
{
  (void)detail::gx_type(input.type());
  auto const n = input.size();
  if (n == 0) return make_empty_column(input.type());
  if (!input.has_nulls()) return copy_of(input, stream, mr);
  detail::result_column out{input.type(), n, true, mask_state::UNINITIALIZED, stream, mr};
  auto const tmp = detail::run_with_scratch(
    [&](void* tmp, std::size_t* bytes) {
      return gx_replace_nulls_policy(static_cast<int>(size_of(input.type())), detail::row0(input), input.null_mask(), input.offset(), n,
                                     policy == replace_policy::FOLLOWING ? 1 : 0, out.data(), out.valid(), out.nulls_dev(), tmp, bytes,
                                     detail::gxs(stream));
    },
    "gx_replace_nulls_policy", stream);
  return out.finish();
}

std::unique_ptr<column> replace_nans(column_view const& input, column_view const& replacement, rmm::cuda_stream_view stream,
                                     rmm::device_async_resource_ref mr)
{
  CUDF_EXPECTS(input.type() == replacement.type(), "Data type mismatch", cudf::data_type_error);
  CUDF_EXPECTS(is_floating_point(input.type()), "nans replacement takes a floating-point column", std::invalid_argument);
  CUDF_EXPECTS(input.size() == replacement.size(), "Column size mismatch", std::invalid_argument);
  if (input.size() == 0) return make_empty_column(input.type());
  return run_replace(true, input, detail::source_of(replacement), stream, mr);
}

std::unique_ptr<column> replace_nans(column_view const& input, scalar const& replacement, rmm::cuda_stream_view stream,
                                     rmm::device_async_resource_ref mr)
{
  CUDF_EXPECTS(input.type() == replacement.type(), "Data type mismatch", cudf::data_type_error);
  CUDF_EXPECTS(is_floating_point(input.type()), "nans replacement takes a floating-point column", std::invalid_argument);
  if (input.size() == 0) return make_empty_column(input.type());
  auto const r = detail::source_of(replacement);
  if (!replacement.is_valid(stream)) return copy_of(input, stream, mr);
  return run_replace(true, input, r, stream, mr);
}

std::unique_ptr<column> find_and_replace_all(column_view const& input, column_view const& values_to_replace,
                                             column_view const& replacement_values, rmm::cuda_stream_view stream,
                                             rmm::device_async_resource_ref mr)
{
  auto const dtype = detail::gx_type(input.type());
  CUDF_EXPECTS(input.type() == values_to_replace.type() && input.type() == replacement_values.type(),
               "Columns type mismatch", cudf::data_type_error);
  CUDF_EXPECTS(values_to_replace.size() == replacement_values.size(), "values_to_replace and replacement_values size mismatch",
               std::invalid_argument);
  CUDF_EXPECTS(!values_to_replace.has_nulls(), "values_to_replace must not have nulls", std::invalid_argument);
  auto const n = input.size();
  if (n == 0) return make_empty_column(input.type());
  if (values_to_replace.size() == 0) return copy_of(input, stream, mr);
  detail::result_column out{input.type(), n, input.has_nulls() || replacement_values.has_nulls(), mask_state::UNINITIALIZED, stream, mr};
  detail::gx_check(gx_find_and_replace(dtype, detail::row0(input), input.has_nulls() ? input.null_mask() : nullptr, input.offset(), n,
                                       detail::row0(values_to_replace), detail::row0(replacement_values),
                                       replacement_values.has_nulls() ? replacement_values.null_mask() : nullptr, replacement_values.offset(),
                                       values_to_replace.size(), out.data(), out.valid(), out.nulls_dev(), detail::gxs(stream)),
                   "gx_find_and_replace");
  return out.finish();
}

std::unique_ptr<column> clamp(column_view const& input, scalar const& lo, scalar const& lo_replace, scalar const& hi,
                              scalar const& hi_replace, rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  auto const dtype = detail::gx_type(input.type());
  CUDF_EXPECTS(lo.type() == hi.type(), "mismatching types of limit scalars", cudf::data_type_error);
  CUDF_EXPECTS(lo_replace.type() == hi_replace.type(), "mismatching types of replace scalars", cudf::data_type_error);
  CUDF_EXPECTS(lo.type() == lo_replace.type(), "mismatching types of limit and replace scalars", cudf::data_type_error);
  CUDF_EXPECTS(lo.type() == input.type(), "mismatching types of scalar and input", cudf::data_type_error);
  auto const n = input.size();
  if (n == 0) return make_empty_column(input.type());
  bool const has_lo = lo.is_valid(stream), has_hi = hi.is_valid(stream);
  if (!has_lo && !has_hi) return copy_of(input, stream, mr);
  if (has_lo) CUDF_EXPECTS(lo_replace.is_valid(stream), "lo_replace can't be null if lo is not null", std::invalid_argument);
  if (has_hi) CUDF_EXPECTS(hi_replace.is_valid(stream), "hi_replace can't be null if hi is not null", std::invalid_argument);
  rmm::device_buffer data{static_cast<std::size_t>(n) * size_of(input.type()), stream, mr};
  detail::gx_check(gx_clamp(dtype, detail::row0(input), n, has_lo ? scalar_device_value(lo) : nullptr, nullptr,
                            has_lo ? scalar_device_value(lo_replace) : nullptr, has_hi ? scalar_device_value(hi) : nullptr, nullptr,
                            has_hi ? scalar_device_value(hi_replace) : nullptr, data.data(), detail::gxs(stream)),
                   "gx_clamp");
  return std::make_unique<column>(input.type(), n, std::move(data), detail::mask_of(input, stream, mr), input.null_count());
}

std::unique_ptr<column> clamp(column_view const& input, scalar const& lo, scalar const& hi, rmm::cuda_stream_view stream,
                              rmm::device_async_resource_ref mr)
{
  return clamp(input, lo, lo, hi, hi, stream, mr);
}

std::unique_ptr<column> normalize_nans_and_zeros(column_view const& input, rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  CUDF_EXPECTS(is_floating_point(input.type()), "Expects float or double input", std::invalid_argument);
  auto const n = input.size();
  if (n == 0) return make_empty_column(input.type());
  rmm::device_buffer data{static_cast<std::size_t>(n) * size_of(input.type()), stream, mr};
  detail::gx_check(gx_normalize_nans_and_zeros(detail::gx_type(input.type()), detail::row0(input), n, data.data(), detail::gxs(stream)),
                   "gx_normalize_nans_and_zeros");
  return std::make_unique<column>(input.type(), n, std::move(data), detail::mask_of(input, stream, mr), input.null_count());
}

void normalize_nans_and_zeros(mutable_column_view& in_out, rmm::cuda_stream_view stream)
{
  CUDF_EXPECTS(is_floating_point(in_out.type()), "Expects float or double input", std::invalid_argument);
  if (in_out.size() == 0) return;
  auto* p = in_out.head<char>() + static_cast<std::size_t>(in_out.offset()) * size_of(in_out.type());
  detail::gx_check(gx_normalize_nans_and_zeros(detail::gx_type(in_out.type()), p, in_out.size(), p, detail::gxs(stream)),
                   "gx_normalize_nans_and_zeros");
}

}  // namespace cudf
