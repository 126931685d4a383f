// cudf::apply_boolean_mask / drop_nulls / drop_nans and cudf::unique / distinct / stable_distinct / distinct_indices / *_count over the
// C ABI (gx_select_* -> gx_compact_column / gx_compact_indices; cudf_amd/csrc/gx_compact.hip, gx_distinct.hip).
// reference: cpp/src/stream_compaction/apply_boolean_mask.cu (apply_boolean_mask), drop_nulls.cu (drop_nulls), drop_nans.cu
// (drop_nans), all three a predicate handed to cudf::detail::copy_if (include/cudf/detail/copy_if.cuh); contract pinned by
// cpp/tests/stream_compaction/apply_boolean_mask_tests.cpp, drop_nulls_tests.cpp, drop_nans_tests.cpp.
// The deduplicating half: cpp/src/stream_compaction/unique.cu, distinct.cu, stable_distinct.cu, distinct_helpers.cu, unique_count.cu,
// distinct_count.cu; contract pinned by cpp/tests/stream_compaction/unique_tests.cpp, distinct_tests.cpp, stable_distinct_tests.cpp,
// unique_count_tests.cpp, distinct_count_tests.cpp.
// A selector writes the plan (selection bits + chunk starts) and the number of kept rows; that count is the one value read back
// before the outputs are allocated, the null counts of all output columns come back in one more read behind the scatters.
#include "ordered_rows.hpp"
#include "result_column.hpp"

#include <cudf/stream_compaction.hpp>

#include <stdexcept>

namespace cudf {
namespace {

// every column of `input` compacted from one plan
std::unique_ptr<table> compact_table(table_view const& input, void const* plan, size_type count, rmm::cuda_stream_view stream,
                                     rmm::device_async_resource_ref mr)
{
  if (count == 0) return detail::empty_like_table(input);
  auto const n = input.num_rows();
  detail::result_table out{input.num_columns(), stream, mr};
  for (auto const& c : input) {
    auto const esz = gx_dtype_size(detail::gx_type(c.type()));
    auto& col      = out.add(c.type(), count, c.has_nulls(), mask_state::ALL_NULL);
    // the kernel writes its count with or without a mask
    detail::gx_check(gx_compact_column(esz, detail::row0(c), c.has_nulls() ? c.null_mask() : nullptr, c.offset(), n, plan, col.data(), col.valid(),
                                       col.count_slot(), detail::gxs(stream)),
                     "gx_compact_column");
  }
  return out.finish(count);
}

// runs a selector (scratch-query convention, the count as a device word in front of it) and compacts the table from its plan
template <typename Selector>
std::unique_ptr<table> select_and_compact(table_view const& input, Selector&& sel, char const* what, rmm::cuda_stream_view stream,
                                          rmm::device_async_resource_ref mr)
{
  rmm::device_uvector<int64_t> count_dev(1, stream);
  auto plan        = detail::run_with_scratch([&](void* t, std::size_t* b) { return sel(count_dev.data(), t, b); }, what, stream);
  auto const count = static_cast<size_type>(detail::read_i64(count_dev.data(), stream));
  return compact_table(input, plan.data(), count, stream, mr);
}

}  // namespace

std::unique_ptr<table> apply_boolean_mask(table_view const& input, column_view const& boolean_mask, rmm::cuda_stream_view stream,
                                          rmm::device_async_resource_ref mr)
{
  if (boolean_mask.is_empty()) return detail::empty_like_table(input);  // (apply_boolean_mask: an empty mask gives empty_like(input))
  CUDF_EXPECTS(input.num_rows() == boolean_mask.size(), "Column size mismatch");
  CUDF_EXPECTS(boolean_mask.type().id() == type_id::BOOL8, "Mask must be Boolean type");
  if (input.num_columns() == 0) return std::make_unique<table>(input, stream, mr);
  auto const n = input.num_rows();
  return select_and_compact(
    input,
    [&](int64_t* cnt, void* t, std::size_t* b) {
      return gx_select_mask(static_cast<uint8_t const*>(detail::row0(boolean_mask)), boolean_mask.has_nulls() ? boolean_mask.null_mask() : nullptr,
                            boolean_mask.offset(), n, cnt, t, b, detail::gxs(stream));
    },
    "apply_boolean_mask", stream, mr);
}

std::unique_ptr<table> drop_nulls(table_view const& input, std::vector<size_type> const& keys, size_type keep_threshold,
                                  rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  auto const key_view = input.select(keys);  // std::out_of_range for an invalid index
  CUDF_EXPECTS(keep_threshold >= 0, "keep_threshold must not be negative", std::invalid_argument);
  if (keys.empty() || input.num_rows() == 0 || !cudf::has_nulls(key_view)) return std::make_unique<table>(input, stream, mr);
  CUDF_EXPECTS(key_view.num_columns() <= detail::MAX_KEYS, "drop_nulls: at most 32 key columns", std::invalid_argument);
  std::vector<uint32_t const*> valid;
  std::vector<int64_t> begin;
  for (auto const& c : key_view) {
    valid.push_back(c.has_nulls() ? c.null_mask() : nullptr);
    begin.push_back(c.offset());
  }
  return select_and_compact(
    input,
    [&](int64_t* cnt, void* t, std::size_t* b) {
      return gx_select_valid_count(static_cast<int>(valid.size()), valid.data(), begin.data(), input.num_rows(), keep_threshold, cnt, t, b,
                                   detail::gxs(stream));
    },
    "drop_nulls", stream, mr);
}

std::unique_ptr<table> drop_nulls(table_view const& input, std::vector<size_type> const& keys, rmm::cuda_stream_view stream,
                                  rmm::device_async_resource_ref mr)
{
  return drop_nulls(input, keys, static_cast<size_type>(keys.size()), stream, mr);
}

std::unique_ptr<table> drop_nans(table_view const& input, std::vector<size_type> const& keys, size_type keep_threshold,
                                 rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  auto const key_view = input.select(keys);  // std::out_of_range for an invalid index
  CUDF_EXPECTS(keep_threshold >= 0, "keep_threshold must not be negative", std::invalid_argument);
  if (input.num_columns() == 0 || input.num_rows() == 0 || keys.empty()) return std::make_unique<table>(input, stream, mr);
  for (auto const& c : key_view) CUDF_EXPECTS(is_floating_point(c.type()), "Key column is not of floating-point type");
  CUDF_EXPECTS(key_view.num_columns() <= detail::MAX_KEYS, "drop_nans: at most 32 key columns", std::invalid_argument);
  auto const dtypes = detail::key_dtypes(key_view);
  detail::key_side const k{key_view};
  return select_and_compact(
    input,
    [&](int64_t* cnt, void* t, std::size_t* b) {
      return gx_select_not_nan(static_cast<int>(dtypes.size()), dtypes.data(), k.data.data(), k.valid.data(), k.begin.data(), k.rows,
                               keep_threshold, /*null_is_missing=*/0, cnt, t, b, detail::gxs(stream));
    },
    "drop_nans", stream, mr);
}

std::unique_ptr<table> drop_nans(table_view const& input, std::vector<size_type> const& keys, rmm::cuda_stream_view stream,
                                 rmm::device_async_resource_ref mr)
{
  return drop_nans(input, keys, static_cast<size_type>(keys.size()), stream, mr);
}

// ---------------------------------------------------------------------------------------------- unique / distinct
namespace {

enum : int { F_NULLS_EQUAL = 1, F_NANS_EQUAL = 2, F_NAN_IS_NULL = 4, F_DROP_NULL_ROWS = 8 };  // flags of gx_select_unique / _distinct

using dedup_fn = int (*)(int, int const*, void const* const*, uint32_t const* const*, int64_t const*, int64_t, int, int, int64_t*, void*,
                         std::size_t*, gx_stream_t);

// the key columns of a deduplicating selector as the host arrays of the C ABI
struct key_arrays {
  std::vector<int> dtypes;
  detail::key_side side;
  explicit key_arrays(table_view const& keys, char const* what) : dtypes{checked_dtypes(keys, what)}, side{keys} {}
  static std::vector<int> checked_dtypes(table_view const& keys, char const* what)
  {
    CUDF_EXPECTS(keys.num_columns() <= detail::MAX_KEYS, std::string{what} + ": at most 32 key columns", std::invalid_argument);
    return detail::key_dtypes(keys);
  }
  int call(dedup_fn fn, int64_t n, int keep, int flags, int64_t* cnt, void* t, std::size_t* b, rmm::cuda_stream_view stream) const
  {
    return fn(static_cast<int>(dtypes.size()), dtypes.data(), side.data.data(), side.valid.data(), side.begin.data(), n, keep, flags, cnt, t, b,
              detail::gxs(stream));
  }
};

int equality_flags(null_equality nulls_equal, nan_equality nans_equal)
{
  return (nulls_equal == null_equality::EQUAL ? F_NULLS_EQUAL : 0) | (nans_equal == nan_equality::ALL_EQUAL ? F_NANS_EQUAL : 0);
}

std::unique_ptr<table> dedup_table(table_view const& input, std::vector<size_type> const& keys, dedup_fn fn, char const* what,
                                   duplicate_keep_option keep, int flags, rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  auto const key_view = input.select(keys);  // std::out_of_range for an invalid index
  if (keys.empty() || input.num_rows() == 0) return std::make_unique<table>(input, stream, mr);
  key_arrays const ka{key_view, what};
  return select_and_compact(
    input,
    [&](int64_t* cnt, void* t, std::size_t* b) { return ka.call(fn, input.num_rows(), static_cast<int>(keep), flags, cnt, t, b, stream); }, what,
    stream, mr);
}

// the number of rows a selector keeps: its count word alone is read, nothing is compacted
size_type dedup_count(table_view const& keys, dedup_fn fn, char const* what, int flags, rmm::cuda_stream_view stream)
{
  if (keys.num_rows() == 0 || keys.num_columns() == 0) return 0;
  key_arrays const ka{keys, what};
  rmm::device_uvector<int64_t> count_dev(1, stream);
  auto scratch = detail::run_with_scratch(
    [&](void* t, std::size_t* b) { return ka.call(fn, keys.num_rows(), GX_KEEP_ANY, flags, count_dev.data(), t, b, stream); }, what, stream);
  return static_cast<size_type>(detail::read_i64(count_dev.data(), stream));
}

int policy_flags(null_policy null_handling, nan_policy nan_handling)
{
  return F_NULLS_EQUAL | F_NANS_EQUAL | (nan_handling == nan_policy::NAN_IS_NULL ? F_NAN_IS_NULL : 0) |
         (null_handling == null_policy::EXCLUDE ? F_DROP_NULL_ROWS : 0);
}

}  // namespace

std::unique_ptr<table> unique(table_view const& input, std::vector<size_type> const& keys, duplicate_keep_option keep,
                              null_equality nulls_equal, rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  return dedup_table(input, keys, gx_select_unique, "unique", keep, equality_flags(nulls_equal, nan_equality::ALL_EQUAL), stream, mr);
}

std::unique_ptr<table> distinct(table_view const& input, std::vector<size_type> const& keys, duplicate_keep_option keep,
                                null_equality nulls_equal, nan_equality nans_equal, rmm::cuda_stream_view stream,
                                rmm::device_async_resource_ref mr)
{
  return dedup_table(input, keys, gx_select_distinct, "distinct", keep, equality_flags(nulls_equal, nans_equal), stream, mr);
}

std::unique_ptr<table> stable_distinct(table_view const& input, std::vector<size_type> const& keys, duplicate_keep_option keep,
                                       null_equality nulls_equal, nan_equality nans_equal, rmm::cuda_stream_view stream,
                                       rmm::device_async_resource_ref mr)
{
  return dedup_table(input, keys, gx_select_distinct, "stable_distinct", keep, equality_flags(nulls_equal, nans_equal), stream, mr);
}

std::unique_ptr<column> distinct_indices(table_view const& input, duplicate_keep_option keep, null_equality nulls_equal,
                                         nan_equality nans_equal, rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  auto const n = input.num_rows();
  if (n == 0 || input.num_columns() == 0) return make_empty_column(data_type{type_id::INT32});
  key_arrays const ka{input, "distinct_indices"};
  rmm::device_uvector<int64_t> count_dev(1, stream);
  auto plan = detail::run_with_scratch(
    [&](void* t, std::size_t* b) {
      return ka.call(gx_select_distinct, n, static_cast<int>(keep), equality_flags(nulls_equal, nans_equal), count_dev.data(), t, b, stream);
    },
    "distinct_indices", stream);
  auto const count = static_cast<size_type>(detail::read_i64(count_dev.data(), stream));
  rmm::device_buffer out{static_cast<std::size_t>(count) * sizeof(int32_t), stream, mr};
  detail::gx_check(gx_compact_indices(n, plan.data(), static_cast<int32_t*>(out.data()), detail::gxs(stream)), "gx_compact_indices");
  return std::make_unique<column>(data_type{type_id::INT32}, count, std::move(out), rmm::device_buffer{0, stream, mr}, 0);
}

size_type unique_count(table_view const& input, null_equality nulls_equal, rmm::cuda_stream_view stream)
{
  return dedup_count(input, gx_select_unique, "unique_count", equality_flags(nulls_equal, nan_equality::ALL_EQUAL), stream);
}

size_type distinct_count(table_view const& input, null_equality nulls_equal, rmm::cuda_stream_view stream)
{
  return dedup_count(input, gx_select_distinct, "distinct_count", equality_flags(nulls_equal, nan_equality::ALL_EQUAL), stream);
}

size_type unique_count(column_view const& input, null_policy null_handling, nan_policy nan_handling, rmm::cuda_stream_view stream)
{
  return dedup_count(table_view{{input}}, gx_select_unique, "unique_count", policy_flags(null_handling, nan_handling), stream);
}

size_type distinct_count(column_view const& input, null_policy null_handling, nan_policy nan_handling, rmm::cuda_stream_view stream)
{
  return dedup_count(table_view{{input}}, gx_select_distinct, "distinct_count", policy_flags(null_handling, nan_handling), stream);
}

}  // namespace cudf
