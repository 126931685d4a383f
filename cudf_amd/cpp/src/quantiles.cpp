// cudf::quantile / cudf::quantiles over the C ABI (gx_quantile_lookup, gx_quantile_index; cudf_amd/csrc/gx_quantile.hip).
// reference: cpp/include/cudf/quantiles.hpp, cpp/src/quantiles/quantile.cu, quantiles.cu -- there one thrust::transform over the
// quantiles; here the lookup kernel with one segment, and for quantiles() sorted_order + gather at host-computed indices.
#include "result_column.hpp"

#include <cudf/copying.hpp>
#include <cudf/quantiles.hpp>
#include <cudf/sorting.hpp>

#include <algorithm>
#include <stdexcept>

namespace cudf {
namespace {

constexpr std::size_t MAX_Q = 64;  // quantiles of one gx_quantile_lookup call

void check_quantiles(std::vector<double> const& q)
{
  for (double x : q)
    if (x != x) throw std::invalid_argument{"quantile: a quantile is NaN"};
}

}  // namespace

std::unique_ptr<column> quantile(column_view const& input, std::vector<double> const& q, interpolation interp,
                                 column_view const& ordered_indices, bool exact, rmm::cuda_stream_view stream,
                                 rmm::device_async_resource_ref mr)
{
  CUDF_EXPECTS(is_numeric(input.type()) && input.type().id() != type_id::BOOL8, "quantile: the input must be numeric and not BOOL8",
               cudf::data_type_error);
  if (!ordered_indices.is_empty() &&
      (ordered_indices.type().id() != type_id::INT32 || ordered_indices.size() != input.size() || ordered_indices.has_nulls()))
    throw std::invalid_argument{"quantile: ordered_indices must be an INT32 column of the input's size without nulls"};
  check_quantiles(q);
  auto const out_type = exact ? data_type{type_id::FLOAT64} : input.type();
  auto const nq       = static_cast<size_type>(q.size());
  if (nq == 0) return make_empty_column(out_type);
  if (input.is_empty()) return make_fixed_width_column(out_type, nq, mask_state::ALL_NULL, stream, mr);
  detail::result_column out{out_type, nq, true, mask_state::ALL_VALID, stream, mr};
  int32_t const offsets_host[2] = {0, input.size()};
  rmm::device_buffer offsets{offsets_host, sizeof(offsets_host), stream};
  auto const w        = size_of(out_type);
  size_type nulls     = 0;
  auto const* order   = ordered_indices.is_empty() ? nullptr
                                                   : static_cast<int32_t const*>(ordered_indices.head<void>()) + ordered_indices.offset();
  for (std::size_t first = 0; first < q.size(); first += MAX_Q) {
    auto const cnt = static_cast<int>(std::min(MAX_Q, q.size() - first));
    // a chunk's validity words start at a word boundary: MAX_Q is a multiple of 32
    detail::gx_check(gx_quantile_lookup(detail::gx_type(input.type()), detail::row0(input), input.has_nulls() ? input.null_mask() : nullptr,
                                        input.offset(), order, 1, static_cast<int32_t const*>(offsets.data()), nullptr, q.data() + first, cnt,
                                        static_cast<int>(interp), exact ? 1 : 0, static_cast<char*>(out.data()) + first * w, out.valid() + first / 32,
                                        out.nulls_dev(), detail::gxs(stream)),
                     "quantile");
    nulls += static_cast<size_type>(detail::read_i64(out.nulls_dev(), stream));  // each chunk overwrites the count
  }
  return out.finish(nulls);
}

std::unique_ptr<table> quantiles(table_view const& input, std::vector<double> const& q, interpolation interp, cudf::sorted is_input_sorted,
                                 std::vector<order> const& column_order, std::vector<null_order> const& null_precedence,
                                 rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  if (interp == interpolation::LINEAR || interp == interpolation::MIDPOINT)
    throw std::invalid_argument{"quantiles: the interpolation must be non-arithmetic (LOWER, HIGHER or NEAREST)"};
  if (input.num_rows() == 0) throw std::invalid_argument{"quantiles: the table has no rows"};
  check_quantiles(q);
  std::vector<int32_t> idx(q.size());
  for (std::size_t j = 0; j < q.size(); ++j) {
    int64_t lower = 0, higher = 0, nearest = 0;
    double frac = 0.0;
    detail::gx_check(gx_quantile_index(input.num_rows(), q[j], &lower, &higher, &nearest, &frac), "quantiles (index)");
    idx[j] = static_cast<int32_t>(interp == interpolation::LOWER ? lower : interp == interpolation::HIGHER ? higher : nearest);
  }
  rmm::device_buffer didx{idx.data(), idx.size() * sizeof(int32_t), stream};
  column_view at{data_type{type_id::INT32}, static_cast<size_type>(idx.size()), didx.data(), nullptr, 0};
  std::unique_ptr<table> result;
  if (is_input_sorted == sorted::YES) {
    result = cudf::gather(input, at, out_of_bounds_policy::DONT_CHECK, stream, mr);
  } else {
    auto order = cudf::sorted_order(input, column_order, null_precedence, stream);
    auto rows  = cudf::gather(table_view{{order->view()}}, at, out_of_bounds_policy::DONT_CHECK, stream);
    result     = cudf::gather(input, rows->get_column(0).view(), out_of_bounds_policy::DONT_CHECK, stream, mr);
  }
  stream.synchronize();  // idx / didx
  return result;
}

}  // namespace cudf
