// cudf::fill / fill_in_place, cudf::repeat and cudf::sequence over the C ABI (gx_fill_range, gx_repeat_each, gx_repeat_map,
// gx_sequence; cudf_amd/csrc/gx_reshape.hip).  reference: cpp/include/cudf/filling.hpp, cpp/src/filling/fill.cu, repeat.cu,
// sequence.cu.  fill writes the range and edits the bitmap (gx_bitmask_copy / gx_bitmask_set).  repeat with a count column casts
// the counts to int64, scans them (so a total of 2^31 or more is seen before anything is sized from it), reads the total once,
// computes one expansion map and gathers every column through it; with a scalar count it is one streaming launch per column.
#include "result_column.hpp"

#include <cudf/copying.hpp>
#include <cudf/filling.hpp>

#include <limits>
#include <stdexcept>
#include <vector>

namespace cudf {
namespace {

constexpr int64_t size_max = std::numeric_limits<size_type>::max();

bool is_integral_not_bool(data_type t)
{
  auto const id = static_cast<int>(t.id());
  return id >= GX_INT8 && id <= GX_UINT64;
}

void check_fill(data_type type, size_type size, size_type begin, size_type end, scalar const& value)
{
  CUDF_EXPECTS(begin >= 0 && end <= size && begin <= end, "Range is out of bounds.", std::out_of_range);
  CUDF_EXPECTS(type == value.type(), "Data type mismatch.", cudf::data_type_error);
  detail::gx_type(type);
  detail::scalar_device_value(value);
}

}  // namespace

void fill_in_place(mutable_column_view& destination, size_type begin, size_type end, scalar const& value, rmm::cuda_stream_view stream)
{
  check_fill(destination.type(), destination.size(), begin, end, value);
  if (begin == end) return;
  bool const valid = value.is_valid(stream);
  CUDF_EXPECTS(valid || destination.nullable(), "destination should be nullable or value should be non-null.", std::invalid_argument);
  auto const esz = static_cast<int>(size_of(destination.type()));
  auto* data     = destination.head<char>() + static_cast<std::size_t>(destination.offset()) * esz;
  if (valid) detail::gx_check(gx_fill_range(esz, data, begin, end, value.device_value_ptr(), detail::gxs(stream)), "gx_fill_range");
  if (destination.nullable()) {
    auto const before = destination.has_nulls() ? destination.null_count(begin, end, stream) : 0;
    detail::gx_check(gx_bitmask_set(destination.null_mask(), static_cast<int64_t>(destination.offset()) + begin,
                                    static_cast<int64_t>(destination.offset()) + end, valid ? 1 : 0, detail::gxs(stream)),
                     "gx_bitmask_set");
    destination.set_null_count(destination.null_count() - before + (valid ? 0 : end - begin));
  }
}

std::unique_ptr<column> fill(column_view const& input, size_type begin, size_type end, scalar const& value, rmm::cuda_stream_view stream,
                             rmm::device_async_resource_ref mr)
{
  check_fill(input.type(), input.size(), begin, end, value);
  if (begin == end) return std::make_unique<column>(input, stream, mr);
  bool const valid = value.is_valid(stream);
  auto const n     = input.size();
  auto const esz   = static_cast<int>(size_of(input.type()));
  rmm::device_buffer data{detail::row0(input), static_cast<std::size_t>(n) * esz, stream, mr};
  if (valid) detail::gx_check(gx_fill_range(esz, data.data(), begin, end, value.device_value_ptr(), detail::gxs(stream)), "gx_fill_range");
  auto const before = input.has_nulls() ? input.null_count(begin, end, stream) : 0;
  auto const nulls  = input.null_count() - before + (valid ? 0 : end - begin);
  rmm::device_buffer mask{0, stream, mr};
  if (nulls > 0) {
    mask        = create_null_mask(n, mask_state::ALL_VALID, stream, mr);
    auto* words = static_cast<uint32_t*>(mask.data());
    if (input.has_nulls())
      detail::gx_check(gx_bitmask_copy(words, 0, input.null_mask(), input.offset(), n, detail::gxs(stream)), "gx_bitmask_copy");
    detail::gx_check(gx_bitmask_set(words, begin, end, valid ? 1 : 0, detail::gxs(stream)), "gx_bitmask_set");
  }
  return std::make_unique<column>(input.type(), n, std::move(data), std::move(mask), nulls);
}

std::unique_ptr<table> repeat(table_view const& input, column_view const& count, rmm::cuda_stream_view stream,
                              rmm::device_async_resource_ref mr)
{
  CUDF_EXPECTS(is_integral_not_bool(count.type()), "count must be an integral column", std::invalid_argument);
  CUDF_EXPECTS(!count.has_nulls(), "count cannot contain nulls", std::invalid_argument);
  CUDF_EXPECTS(input.num_rows() == count.size(), "in and count must have equal size", std::invalid_argument);
  for (auto const& c : input) detail::gx_type(c.type());
  auto const n = input.num_rows();
  if (n == 0) return detail::empty_like_table(input);
  // counts as int64 with one 0 behind them: the exclusive scan of n + 1 entries ends in the total
  auto const n1 = static_cast<std::size_t>(n) + 1;
  rmm::device_uvector<int64_t> counts(n1, stream), offsets64(n1, stream);
  CUDF_CUDA_TRY(hipMemsetAsync(counts.data() + n, 0, sizeof(int64_t), stream.value()));
  detail::gx_check(gx_cast(detail::gx_type(count.type()), detail::row0(count), n, GX_INT64, counts.data(), detail::gxs(stream)), "gx_cast");
  auto scan_tmp = detail::run_with_scratch(
    [&](void* t, std::size_t* b) {
      return gx_scan(GX_INT64, counts.data(), nullptr, static_cast<int64_t>(n1), 0 /* sum */, 0, offsets64.data(), t, b, detail::gxs(stream));
    },
    "gx_scan", stream);
  auto const total = detail::read_i64(offsets64.data() + n, stream);  // the one host read: it sizes the result
  CUDF_EXPECTS(total <= size_max, "The repeated rows exceed the column size limit", std::overflow_error);
  if (total <= 0) return detail::empty_like_table(input);
  rmm::device_uvector<int32_t> offsets(n1, stream), map(static_cast<std::size_t>(total), stream);
  detail::gx_check(gx_cast(GX_INT64, offsets64.data(), static_cast<int64_t>(n1), GX_INT32, offsets.data(), detail::gxs(stream)), "gx_cast");
  auto map_tmp = detail::run_with_scratch(
    [&](void* t, std::size_t* b) { return gx_repeat_map(offsets.data(), n, total, map.data(), t, b, detail::gxs(stream)); }, "gx_repeat_map",
    stream);
  column_view const map_view{data_type{type_id::INT32}, static_cast<size_type>(total), map.data(), nullptr, 0};
  auto cols = gather(input, map_view, out_of_bounds_policy::DONT_CHECK, stream, mr)->release();
  for (auto& c : cols)
    if (c->nullable() && c->null_count() == 0) c->set_null_mask(rmm::device_buffer{0, stream, mr}, 0);
  return std::make_unique<table>(std::move(cols));
}

std::unique_ptr<table> repeat(table_view const& input, size_type count, rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  return detail::tile_or_repeat_each(true, input, count, stream, mr);
}

std::unique_ptr<column> sequence(size_type size, scalar const& init, scalar const& step, rmm::cuda_stream_view stream,
                                 rmm::device_async_resource_ref mr)
{
  CUDF_EXPECTS(init.type() == step.type(), "init and step must be of the same type.", cudf::data_type_error);
  CUDF_EXPECTS(size >= 0, "size must be >= 0", std::invalid_argument);
  auto const id = static_cast<int>(init.type().id());
  CUDF_EXPECTS(id >= GX_INT8 && id <= GX_FLOAT64, "Input scalar types must be numeric", std::invalid_argument);
  CUDF_EXPECTS(init.is_valid(stream) && step.is_valid(stream), "init and step must be valid", std::invalid_argument);
  if (size == 0) return make_empty_column(init.type());
  rmm::device_buffer data{static_cast<std::size_t>(size) * size_of(init.type()), stream, mr};
  detail::gx_check(gx_sequence(id, data.data(), size, init.device_value_ptr(), step.device_value_ptr(), detail::gxs(stream)), "gx_sequence");
  return std::make_unique<column>(init.type(), size, std::move(data), rmm::device_buffer{0, stream, mr}, 0);
}

std::unique_ptr<column> sequence(size_type size, scalar const& init, rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  CUDF_EXPECTS(size >= 0, "size must be >= 0", std::invalid_argument);
  auto const id = static_cast<int>(init.type().id());
  CUDF_EXPECTS(id >= GX_INT8 && id <= GX_FLOAT64, "Input scalar types must be numeric", std::invalid_argument);
  CUDF_EXPECTS(init.is_valid(stream), "init must be valid", std::invalid_argument);
  if (size == 0) return make_empty_column(init.type());
  rmm::device_buffer data{static_cast<std::size_t>(size) * size_of(init.type()), stream, mr};
  detail::gx_check(gx_sequence(id, data.data(), size, init.device_value_ptr(), nullptr, detail::gxs(stream)), "gx_sequence");
  return std::make_unique<column>(init.type(), size, std::move(data), rmm::device_buffer{0, stream, mr}, 0);
}

}  // namespace cudf
