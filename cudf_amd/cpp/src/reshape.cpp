// cudf::interleave_columns, cudf::tile and cudf::transpose over the C ABI (gx_interleave, gx_tile; cudf_amd/csrc/gx_reshape.hip).
// reference: cpp/include/cudf/reshape.hpp, cpp/include/cudf/transpose.hpp, cpp/src/reshape/interleave_columns.cu, tile.cu,
// cpp/src/transpose/transpose.cu.  One launch writes values, validity words and the null count; sliced views are read in place
// (offset data pointer, begin bit).  A mask is allocated only when an input has nulls and kept only when the result does: the one
// host read of these paths.  transpose is the interleave plus views: its per-view null counts come from one copy of the bitmap.
#include "common.hpp"

#include <cudf/column/column_factories.hpp>
#include <cudf/null_mask.hpp>
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
  rmm::device_buffer data{static_cast<std::size_t>(total) * esz, stream, mr};
  auto mask = create_null_mask(total, with_mask ? mask_state::UNINITIALIZED : mask_state::UNALLOCATED, stream, mr);
  rmm::device_buffer nulls_dev{sizeof(int64_t), stream};
  auto scratch = detail::run_with_scratch(
    [&](void* t, std::size_t* b) {
      return gx_interleave(esz, k, cols.data(), valid.data(), bits.data(), n, data.data(), with_mask ? static_cast<uint32_t*>(mask.data()) : nullptr,
                           with_mask ? static_cast<int64_t*>(nulls_dev.data()) : nullptr, t, b, detail::gxs(stream));
    },
    "gx_interleave", stream);
  auto const nulls = with_mask ? static_cast<size_type>(detail::read_i64(static_cast<int64_t const*>(nulls_dev.data()), stream)) : 0;
  return std::make_unique<column>(type, total, std::move(data), nulls > 0 ? std::move(mask) : rmm::device_buffer{0, stream, mr}, nulls);
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
  std::vector<std::unique_ptr<column>> cols;
  cols.reserve(nc);
  if (total == 0) {
    for (auto const& c : input) cols.emplace_back(make_empty_column(c.type()));
    return std::make_unique<table>(std::move(cols));
  }
  struct part {
    rmm::device_buffer data, mask;
    bool with_mask;
  };
  std::vector<part> parts;
  parts.reserve(nc);
  rmm::device_uvector<int64_t> counts_dev(static_cast<std::size_t>(std::max<size_type>(nc, 1)), stream);
  bool any_mask = false;
  for (size_type k = 0; k < nc; ++k) {
    auto const& c  = input.column(k);
    auto const esz = static_cast<int>(size_of(c.type()));
    part p{rmm::device_buffer{static_cast<std::size_t>(total) * esz, stream, mr},
           create_null_mask(total, c.has_nulls() ? mask_state::UNINITIALIZED : mask_state::UNALLOCATED, stream, mr), c.has_nulls()};
    auto* out_valid = p.with_mask ? static_cast<uint32_t*>(p.mask.data()) : nullptr;
    auto* out_nulls = p.with_mask ? counts_dev.data() + k : nullptr;
    auto const* iv  = p.with_mask ? c.null_mask() : nullptr;
    if (each)
      gx_check(gx_repeat_each(esz, row0(c), iv, c.offset(), n, count, p.data.data(), out_valid, out_nulls, gxs(stream)), "gx_repeat_each");
    else
      gx_check(gx_tile(esz, row0(c), iv, c.offset(), n, count, p.data.data(), out_valid, out_nulls, gxs(stream)), "gx_tile");
    any_mask |= p.with_mask;
    parts.emplace_back(std::move(p));
  }
  std::vector<int64_t> nulls(static_cast<std::size_t>(nc), 0);
  if (any_mask) {  // all counts in one read (entries of columns without a mask are not written and not used)
    CUDF_CUDA_TRY(hipMemcpyAsync(nulls.data(), counts_dev.data(), nulls.size() * sizeof(int64_t), hipMemcpyDeviceToHost, stream.value()));
    stream.synchronize();
  }
  for (size_type k = 0; k < nc; ++k) {
    auto& p      = parts[k];
    auto const z = p.with_mask ? static_cast<size_type>(nulls[k]) : 0;
    cols.emplace_back(std::make_unique<column>(input.column(k).type(), total, std::move(p.data),
                                               z > 0 ? std::move(p.mask) : rmm::device_buffer{0, stream, mr}, z));
  }
  return std::make_unique<table>(std::move(cols));
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
