// cudf::interleave_columns, cudf::tile and cudf::transpose over the C ABI (gx_interleave, gx_tile; cudf_amd/csrc/gx_reshape.hip).
// reference: cpp/include/cudf/reshape.hpp, cpp/include/cudf/transpose.hpp, cpp/src/reshape/interleave_columns.cu, tile.cu,
// cpp/src/transpose/transpose.cu.  One launch writes values, validity words and the null count; sliced views are read in place
// (offset data pointer, begin bit); the result mask follows the contract of DESIGN.md 3.6 (result_column.hpp).
// transpose is the interleave plus views: its per-view null counts come from one copy of the bitmap.
#include "result_column.hpp"

#include <cudf/reshape.hpp>
#include <cudf/transpose.hpp>

#include <algorithm>
#include <limits>
#include <stdexcept>
#include <vector>

namespace cudf {
namespace {

constexpr int64_t size_max = std::numeric_limits<size_type>::max();

// the type all columns share (EMPTY for no columns); cudf::data_type_error when they differ or are not fixed-width
data_type common_type(table_view const& input)
{
  if (input.num_columns() == 0) return data_type{type_id::EMPTY};
  auto const type = input.column(0).type();
  for (auto const& c : input) CUDF_EXPECTS(c.type() == type, "The columns differ in type", cudf::data_type_error);
  detail::gx_type(type);
  return type;
}

std::unique_ptr<column> interleave(table_view const& input, data_type type, rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  auto const k = input.num_columns();
  auto const n = input.num_rows();
  CUDF_EXPECTS(static_cast<int64_t>(n) * k <= size_max, "The interleaved column exceeds the column size limit", std::overflow_error);
  if (n == 0) return make_empty_column(type);
  auto const esz   = static_cast<int>(size_of(type));
  auto const total = static_cast<size_type>(n * k);
  std::vector<void const*> cols(k);
  std::vector<uint32_t const*> valid(k);
  std::vector<int64_t> bits(k);
  bool with_mask = false;
  for (size_type j = 0; j < k; ++j) {
    auto const& c = input.column(j);
    cols[j]       = detail::row0(c);
    valid[j]      = c.has_nulls() ? c.null_mask() : nullptr;
    bits[j]       = c.offset();
    with_mask |= c.has_nulls();
  }
  detail::result_column out{type, total, with_mask, mask_state::UNINITIALIZED, stream, mr};
  auto scratch = detail::run_with_scratch(
    [&](void* t, std::size_t* b) {
      return gx_interleave(esz, k, cols.data(), valid.data(), bits.data(), n, out.data(), out.valid(), out.nulls_dev(), t, b, detail::gxs(stream));
    },
    "gx_interleave", stream);
  return out.finish();
}

}  // namespace

namespace detail {

std::unique_ptr<table> tile_or_repeat_each(bool each, table_view const& input, size_type count, rmm::cuda_stream_view stream,
                                           rmm::device_async_resource_ref mr)
{
  CUDF_EXPECTS(count >= 0, "count cannot be negative", std::invalid_argument);
  auto const n  = input.num_rows();
  auto const nc = input.num_columns();
  CUDF_EXPECTS(static_cast<int64_t>(n) * count <= size_max, "The result exceeds the column size limit", std::overflow_error);
  for (auto const& c : input) gx_type(c.type());
  auto const total = static_cast<size_type>(n * count);
  if (total == 0) return empty_like_table(input);
  result_table out{nc, stream, mr};
  for (auto const& c : input) {
    auto const esz = static_cast<int>(size_of(c.type()));
    auto& col      = out.add(c.type(), total, c.has_nulls(), mask_state::UNINITIALIZED);
    auto const* iv = c.has_nulls() ? c.null_mask() : nullptr;
    if (each)
      gx_check(gx_repeat_each(esz, row0(c), iv, c.offset(), n, count, col.data(), col.valid(), col.nulls_dev(), gxs(stream)), "gx_repeat_each");
    else
      gx_check(gx_tile(esz, row0(c), iv, c.offset(), n, count, col.data(), col.valid(), col.nulls_dev(), gxs(stream)), "gx_tile");
  }
  return out.finish(total);
}

}  // namespace detail

std::unique_ptr<column> interleave_columns(table_view const& input, rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  CUDF_EXPECTS(input.num_columns() > 0, "input must have at least one column to determine dtype.", std::invalid_argument);
  return interleave(input, common_type(input), stream, mr);
}

std::unique_ptr<table> tile(table_view const& input, size_type count, rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  return detail::tile_or_repeat_each(false, input, count, stream, mr);
}

std::pair<std::unique_ptr<column>, table_view> transpose(table_view const& input, rmm::cuda_stream_view stream,
                                                         rmm::device_async_resource_ref mr)
{
  auto const type = common_type(input);
  auto const k    = input.num_columns();
  auto const n    = input.num_rows();
  if (k == 0 || n == 0) return std::make_pair(std::make_unique<column>(), table_view{});
  auto whole      = interleave(input, type, stream, mr);
  auto const view = whole->view();
  // nulls of each result column: bits [i * k, (i + 1) * k) of the bitmap, counted on the host from one copy of its words
  std::vector<size_type> nulls(static_cast<std::size_t>(n), 0);
  if (whole->null_count() > 0) {
    std::vector<bitmask_type> words(static_cast<std::size_t>(num_bitmask_words(view.size())));
    CUDF_CUDA_TRY(hipMemcpyAsync(words.data(), view.null_mask(), words.size() * sizeof(bitmask_type), hipMemcpyDeviceToHost, stream.value()));
    stream.synchronize();
    for (size_type i = 0; i < n; ++i) {
      int64_t const b0 = static_cast<int64_t>(i) * k, b1 = b0 + k;
      size_type set = 0;
      for (int64_t w = b0 >> 5; w <= (b1 - 1) >> 5; ++w) {
        bitmask_type m  = words[static_cast<std::size_t>(w)];
        int64_t const lo = w * 32, hi = lo + 32;
        if (b0 > lo) m &= 0xFFFFFFFFu << (b0 - lo);
        if (b1 < hi) m &= 0xFFFFFFFFu >> (hi - b1);
        set += __builtin_popcount(m);
      }
      nulls[static_cast<std::size_t>(i)] = k - set;
    }
  }
  std::vector<column_view> cols;
  cols.reserve(n);
  for (size_type i = 0; i < n; ++i)
    cols.emplace_back(type, k, view.head<void>(), view.null_mask(), nulls[static_cast<std::size_t>(i)], i * k);
  return std::make_pair(std::move(whole), table_view{cols});
}

}  // namespace cudf
