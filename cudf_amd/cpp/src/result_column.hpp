// result_column.hpp -- the two models every value entry point of the host library shares:
//  * result_column / result_table: the column(s) a launch writes as values, validity words and a device null count.  A mask is
//    allocated only when the result can hold a null, the count is read only when there is a mask, the mask is kept only when a row
//    is null.
//  * source: a column view or a device scalar as a kernel operand.  Building one makes no device call; a scalar's validity is read
//    by scalar_may_be_null, which the caller takes after its argument checks.
#pragma once
#include "common.hpp"

#include <cudf/column/column_factories.hpp>
#include <cudf/null_mask.hpp>
#include <cudf/scalar/scalar.hpp>

#include <algorithm>
#include <vector>

namespace cudf {
namespace detail {

class result_column {
 public:
  // `state` is what the kernel expects of the words it is handed (UNINITIALIZED: it writes every word; ALL_NULL / ALL_VALID: it
  // clears / sets bits).  `shared_count`: a slot of a caller-owned counts array (result_table) in place of the private one.
  result_column(data_type type, size_type rows, bool with_mask, mask_state state, rmm::cuda_stream_view stream,
                rmm::device_async_resource_ref mr, int64_t* shared_count = nullptr)
    : result_column(type, rows, rmm::device_buffer{static_cast<std::size_t>(rows) * size_of(type), stream, mr}, with_mask, state, stream, mr,
                    shared_count)
  {
  }
  // the same over values the caller has already placed (scatter: a copy of the target)
  result_column(data_type type, size_type rows, rmm::device_buffer&& data, bool with_mask, mask_state state, rmm::cuda_stream_view stream,
                rmm::device_async_resource_ref mr, int64_t* shared_count = nullptr)
    : _type{type},
      _rows{rows},
      _with_mask{with_mask},
      _stream{stream},
      _mr{mr},
      _data{std::move(data)},
      _mask{create_null_mask(rows, with_mask ? state : mask_state::UNALLOCATED, stream, mr)},
      _own_count{shared_count ? 0 : sizeof(int64_t), stream},
      _count{shared_count ? shared_count : static_cast<int64_t*>(_own_count.data())}
  {
  }

  [[nodiscard]] bool with_mask() const { return _with_mask; }
  [[nodiscard]] void* data() { return _data.data(); }
  [[nodiscard]] uint32_t* valid() { return _with_mask ? static_cast<uint32_t*>(_mask.data()) : nullptr; }
  [[nodiscard]] int64_t* nulls_dev() { return _with_mask ? _count : nullptr; }
  [[nodiscard]] int64_t* count_slot() { return _count; }  // for a kernel that writes its count with or without a mask

  // the one host read of the path, and only with a mask
  std::unique_ptr<column> finish() { return finish(_with_mask ? static_cast<size_type>(read_i64(_count, _stream)) : 0); }
  // for a caller that has the count already
  std::unique_ptr<column> finish(size_type nulls)
  {
    return std::make_unique<column>(_type, _rows, std::move(_data), nulls > 0 ? std::move(_mask) : rmm::device_buffer{0, _stream, _mr}, nulls);
  }

 private:
  data_type _type;
  size_type _rows;
  bool _with_mask;
  rmm::cuda_stream_view _stream;
  rmm::device_async_resource_ref _mr;
  rmm::device_buffer _data, _mask, _own_count;
  int64_t* _count;
};

// The columns of a result table, one launch each: their counts share one array and come back in one copy behind the last launch,
// and in none when no column has a mask.
class result_table {
 public:
  result_table(size_type num_columns, rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
    : _stream{stream}, _mr{mr}, _counts(static_cast<std::size_t>(std::max<size_type>(num_columns, 1)), stream)
  {
    _cols.reserve(num_columns);
  }

  result_column& add(data_type type, size_type rows, bool with_mask, mask_state state)
  {
    return _cols.emplace_back(type, rows, with_mask, state, _stream, _mr, _counts.data() + _cols.size());
  }
  result_column& add(data_type type, size_type rows, rmm::device_buffer&& data, bool with_mask, mask_state state)
  {
    return _cols.emplace_back(type, rows, std::move(data), with_mask, state, _stream, _mr, _counts.data() + _cols.size());
  }

  // counts_are_set_bits: the kernels counted valid rows (scatter), so nulls = rows - count
  std::unique_ptr<table> finish(size_type rows, bool counts_are_set_bits = false)
  {
    std::vector<int64_t> counts(_cols.size(), 0);
    if (std::any_of(_cols.begin(), _cols.end(), [](auto const& c) { return c.with_mask(); })) {
      // entries of columns without a mask may be unwritten and are not used
      CUDF_CUDA_TRY(hipMemcpyAsync(counts.data(), _counts.data(), counts.size() * sizeof(int64_t), hipMemcpyDeviceToHost, _stream.value()));
      _stream.synchronize();
    }
    std::vector<std::unique_ptr<column>> out;
    out.reserve(_cols.size());
    for (std::size_t k = 0; k < _cols.size(); ++k) {
      auto const nulls = !_cols[k].with_mask() ? 0 : static_cast<size_type>(counts_are_set_bits ? rows - counts[k] : counts[k]);
      out.emplace_back(_cols[k].finish(nulls));
    }
    return std::make_unique<table>(std::move(out));
  }

 private:
  rmm::cuda_stream_view _stream;
  rmm::device_async_resource_ref _mr;
  rmm::device_uvector<int64_t> _counts;
  std::vector<result_column> _cols;
};

// validity of a per-group result from the number of valid values that went into each group
inline void mask_from_counts(column& c, int32_t const* counts, rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  auto const g            = c.size();
  rmm::device_buffer mask = create_null_mask(g, mask_state::ALL_VALID, stream, mr);
  rmm::device_buffer cnt{sizeof(int64_t), stream};
  gx_check(gx_valid_from_counts(counts, g, static_cast<uint32_t*>(mask.data()), static_cast<int64_t*>(cnt.data()), gxs(stream)), "groupby validity");
  auto const nulls = static_cast<size_type>(read_i64(static_cast<int64_t const*>(cnt.data()), stream));
  if (nulls > 0) c.set_null_mask(std::move(mask), nulls);
}

// One operand of a kernel: a column view read in place (offset data pointer, begin bit) or a scalar whose value and validity byte
// stay on the device.
struct source {
  void const* data{nullptr};
  uint32_t const* valid{nullptr};
  int64_t begin_bit{0};
  uint8_t const* scalar_valid{nullptr};
  int is_scalar{0};
  bool may_be_null{false};
  data_type type{type_id::EMPTY};
  [[nodiscard]] int dtype() const { return static_cast<int>(type.id()); }
};

inline source source_of(column_view const& c)
{
  gx_type(c.type());
  return {row0(c), c.has_nulls() ? c.null_mask() : nullptr, c.offset(), nullptr, 0, c.has_nulls(), c.type()};
}

// device address of a fixed-width scalar's value
inline void const* scalar_device_value(scalar const& s)
{
  auto const* p = s.device_value_ptr();
  CUDF_EXPECTS(p != nullptr, "Only fixed-width scalars are supported on this path", cudf::data_type_error);
  return p;
}

// no device call: may_be_null stays false until the caller asks scalar_may_be_null
inline source source_of(scalar const& s)
{
  gx_type(s.type());
  return {scalar_device_value(s), nullptr, 0, reinterpret_cast<uint8_t const*>(s.validity_data()), 1, false, s.type()};
}

// the device read that decides whether a scalar operand asks for a result mask: after every argument check, and not without rows
inline bool scalar_may_be_null(scalar const& s, bool have_rows, rmm::cuda_stream_view stream) { return have_rows && !s.is_valid(stream); }

}  // namespace detail
}  // namespace cudf
