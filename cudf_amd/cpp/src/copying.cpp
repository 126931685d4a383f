// cudf::concatenate / concatenate_masks, cudf::scatter, cudf::copy_if_else, cudf::slice and cudf::split over the C ABI
// (gx_concatenate, gx_scatter, gx_copy_if_else; cudf_amd/csrc/gx_copying.hip).
// reference: cpp/include/cudf/concatenate.hpp + src/copying/concatenate.cu (a fused kernel up to a byte limit, else one copy and
// one mask kernel per input), include/cudf/copying.hpp + detail/scatter.cuh, detail/copy_if_else.cuh, src/copying/slice.cu,
// split.cpp.  Here concatenate is one fused launch for any number of inputs (data, validity words and sliced views in the same
// pass) whose null count is the sum of the views' null counts: nothing is read back.  scatter copies the target and writes in
// place; its null counts come back in one read behind the last column.  slice and split only make views.  Operands and result
// masks of scatter and copy_if_else follow the models of DESIGN.md 3.6 (result_column.hpp).
#include "result_column.hpp"

#include <cudf/concatenate.hpp>
#include <cudf/copying.hpp>

#include <algorithm>
#include <limits>
#include <stdexcept>
#include <vector>

namespace cudf {
namespace {

// type, row total and null total of the inputs of a concatenate, with its throws: all decided on the host
struct concat_plan {
  data_type type{type_id::EMPTY};
  int64_t rows{0};
  int64_t nulls{0};
  bool any_nullable{false};
};

concat_plan plan_of(host_span<column_view const> views, bool same_type)
{
  CUDF_EXPECTS(views.size() > 0, "Unexpected empty list of columns to concatenate.", std::invalid_argument);
  concat_plan p;
  p.type = views[0].type();
  for (auto const& c : views) {
    if (same_type) CUDF_EXPECTS(c.type() == p.type, "Type mismatch in columns to concatenate.", cudf::data_type_error);
    p.rows += c.size();
    p.nulls += c.null_count();
    p.any_nullable |= c.nullable();
  }
  CUDF_EXPECTS(p.rows <= static_cast<int64_t>(std::numeric_limits<size_type>::max()),
               "Total number of concatenated rows exceeds the column size limit", std::overflow_error);
  return p;
}

// the fused launch: data (unless data == nullptr) and validity (unless mask == nullptr) of the concatenation of `views`
void run_concatenate(host_span<column_view const> views, int elem_size, void* data, uint32_t* mask, rmm::cuda_stream_view stream)
{
  auto const k = views.size();
  std::vector<void const*> cols(k);
  std::vector<int64_t> rows(k), bits(k);
  std::vector<uint32_t const*> valid(k);
  for (std::size_t i = 0; i < k; ++i) {
    auto const& c = views[i];
    cols[i]       = data ? static_cast<char const*>(c.head<void>()) + static_cast<std::size_t>(c.offset()) * elem_size : nullptr;
    rows[i]       = c.size();
    valid[i]      = c.nullable() && (c.has_nulls() || !data) ? c.null_mask() : nullptr;
    bits[i]       = c.offset();
  }
  auto scratch = detail::run_with_scratch(
    [&](void* t, std::size_t* b) {
      return gx_concatenate(elem_size, static_cast<int>(k), data ? cols.data() : nullptr, rows.data(), valid.data(), bits.data(), data, mask,
                            nullptr, t, b, detail::gxs(stream));
    },
    "gx_concatenate", stream);
}

void check_map(column_view const& map, char const* what)
{
  CUDF_EXPECTS(not map.has_nulls() && not map.nullable(), std::string{what} + " contains nulls", std::invalid_argument);
  CUDF_EXPECTS(map.type().id() == type_id::INT32, std::string{what} + " must be an INT32 column", cudf::data_type_error);
}

using detail::source;

// column k of a scatter: a copy of `target` with the n rows of map written from `src`; the kernel leaves the count of SET bits
void scatter_column(detail::result_table& out, source const& src, int32_t const* map, size_type n, column_view const& target,
                    rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  auto const esz  = static_cast<int>(size_of(target.type()));
  auto const rows = target.size();
  auto& col       = out.add(target.type(), rows, rmm::device_buffer{detail::row0(target), static_cast<std::size_t>(rows) * esz, stream, mr},
                            target.has_nulls() || src.may_be_null, mask_state::ALL_VALID);
  if (target.has_nulls()) run_concatenate(host_span<column_view const>{&target, 1}, esz, nullptr, col.valid(), stream);
  if (n > 0) {
    detail::gx_check(gx_scatter(esz, src.data, src.valid, src.begin_bit, src.scalar_valid, src.is_scalar, map, n, col.data(), col.valid(), rows,
                                detail::gxs(stream)),
                     "gx_scatter");
  }
  if (col.with_mask())
    detail::gx_check(gx_bitmask_count(col.valid(), 0, rows, col.nulls_dev(), detail::gxs(stream)), "scatter null count");
}

std::unique_ptr<column> select(source const& lhs, source const& rhs, column_view const& boolean_mask, rmm::cuda_stream_view stream,
                               rmm::device_async_resource_ref mr)
{
  auto const n   = boolean_mask.size();
  auto const esz = static_cast<int>(size_of(lhs.type));
  if (n == 0) return make_empty_column(lhs.type);
  detail::result_column out{lhs.type, n, lhs.may_be_null || rhs.may_be_null, mask_state::UNINITIALIZED, stream, mr};
  detail::gx_check(gx_copy_if_else(esz, lhs.data, lhs.valid, lhs.begin_bit, lhs.scalar_valid, lhs.is_scalar, rhs.data, rhs.valid,
                                   rhs.begin_bit, rhs.scalar_valid, rhs.is_scalar, static_cast<uint8_t const*>(detail::row0(boolean_mask)),
                                   boolean_mask.has_nulls() ? boolean_mask.null_mask() : nullptr, boolean_mask.offset(), n, out.data(),
                                   out.valid(), out.nulls_dev(), detail::gxs(stream)),
                   "gx_copy_if_else");
  return out.finish();
}

// a scalar side, built after check_select: its validity is the device read that decides whether the result needs a mask
source checked_source_of(scalar const& s, bool have_rows, rmm::cuda_stream_view stream)
{
  auto o        = detail::source_of(s);
  o.may_be_null = detail::scalar_may_be_null(s, have_rows, stream);
  return o;
}

void check_select(data_type lhs, data_type rhs, column_view const& boolean_mask)
{
  CUDF_EXPECTS(boolean_mask.type().id() == type_id::BOOL8, "Boolean mask column must be of type type_id::BOOL8", cudf::data_type_error);
  CUDF_EXPECTS(lhs == rhs, "Both inputs must be of the same type", cudf::data_type_error);
  detail::gx_type(lhs);
}

void check_slice_indices(size_type size, host_span<size_type const> indices)
{
  CUDF_EXPECTS(indices.size() % 2 == 0, "indices size must be even", std::invalid_argument);
  for (std::size_t i = 0; i < indices.size(); i += 2) {
    auto const begin = indices[i], end = indices[i + 1];
    CUDF_EXPECTS(begin >= 0, "Starting index cannot be negative.", std::out_of_range);
    CUDF_EXPECTS(end >= 0, "End index cannot be negative.", std::out_of_range);
    CUDF_EXPECTS(end >= begin, "End index cannot be smaller than the starting index.", std::invalid_argument);
    CUDF_EXPECTS(end <= size, "Slice range out of bounds.", std::out_of_range);
  }
}

std::vector<size_type> split_to_slice_indices(size_type size, host_span<size_type const> splits)
{
  std::vector<size_type> indices;
  indices.reserve(2 * (splits.size() + 1));
  size_type begin = 0;
  for (auto s : splits) {
    indices.push_back(begin);
    indices.push_back(s);
    begin = s;
  }
  indices.push_back(begin);
  indices.push_back(size);
  return indices;
}

}  // namespace

// ------------------------------------------------------------------------------------ concatenate
std::unique_ptr<column> concatenate(host_span<column_view const> columns_to_concat, rmm::cuda_stream_view stream,
                                    rmm::device_async_resource_ref mr)
{
  auto const p   = plan_of(columns_to_concat, true);
  auto const esz = gx_dtype_size(detail::gx_type(p.type));
  if (p.rows == 0) return make_empty_column(p.type);
  auto const n = static_cast<size_type>(p.rows);
  rmm::device_buffer data{static_cast<std::size_t>(n) * esz, stream, mr};
  bool const with_mask = p.nulls > 0;
  auto mask            = create_null_mask(n, with_mask ? mask_state::UNINITIALIZED : mask_state::UNALLOCATED, stream, mr);
  run_concatenate(columns_to_concat, esz, data.data(), with_mask ? static_cast<uint32_t*>(mask.data()) : nullptr, stream);
  return std::make_unique<column>(p.type, n, std::move(data), std::move(mask), static_cast<size_type>(p.nulls));
}

std::unique_ptr<table> concatenate(host_span<table_view const> tables_to_concat, rmm::cuda_stream_view stream,
                                   rmm::device_async_resource_ref mr)
{
  CUDF_EXPECTS(tables_to_concat.size() > 0, "Unexpected empty list of tables to concatenate.", std::invalid_argument);
  auto const nc = tables_to_concat[0].num_columns();
  for (auto const& t : tables_to_concat) CUDF_EXPECTS(t.num_columns() == nc, "Mismatch in table columns to concatenate.");
  std::vector<std::vector<column_view>> per_column(static_cast<std::size_t>(nc));
  for (size_type k = 0; k < nc; ++k) {
    for (auto const& t : tables_to_concat) per_column[k].push_back(t.column(k));
    plan_of(per_column[k], true);  // every throw before the first launch
    detail::gx_type(per_column[k][0].type());
  }
  std::vector<std::unique_ptr<column>> cols;
  cols.reserve(nc);
  for (size_type k = 0; k < nc; ++k) cols.emplace_back(concatenate(host_span<column_view const>{per_column[k]}, stream, mr));
  return std::make_unique<table>(std::move(cols));
}

rmm::device_buffer concatenate_masks(host_span<column_view const> views, rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  auto const p = plan_of(views, false);
  if (!p.any_nullable || p.rows == 0) return rmm::device_buffer{0, stream, mr};
  auto const n = static_cast<size_type>(p.rows);
  auto mask    = create_null_mask(n, mask_state::UNINITIALIZED, stream, mr);
  run_concatenate(views, 1, nullptr, static_cast<uint32_t*>(mask.data()), stream);
  return mask;
}

// ------------------------------------------------------------------------------------ scatter
std::unique_ptr<table> scatter(table_view const& source, column_view const& scatter_map, table_view const& target,
                               rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  CUDF_EXPECTS(source.num_columns() == target.num_columns(), "Number of columns in source and target not equal");
  CUDF_EXPECTS(scatter_map.size() <= source.num_rows(), "Size of scatter map must be equal to or less than source rows");
  check_map(scatter_map, "scatter_map");
  for (size_type k = 0; k < source.num_columns(); ++k) {
    CUDF_EXPECTS(source.column(k).type() == target.column(k).type(), "Column types do not match between source and target", cudf::data_type_error);
    detail::gx_type(target.column(k).type());
  }
  detail::result_table out{target.num_columns(), stream, mr};
  auto const* map = static_cast<int32_t const*>(detail::row0(scatter_map));
  for (size_type k = 0; k < target.num_columns(); ++k)
    scatter_column(out, detail::source_of(source.column(k)), map, scatter_map.size(), target.column(k), stream, mr);
  return out.finish(target.num_rows(), true);
}

std::unique_ptr<table> scatter(std::vector<std::reference_wrapper<scalar const>> const& source, column_view const& indices,
                               table_view const& target, rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  CUDF_EXPECTS(static_cast<size_type>(source.size()) == target.num_columns(), "Number of scalars and table columns mismatch");
  check_map(indices, "indices");
  for (size_type k = 0; k < target.num_columns(); ++k) {
    CUDF_EXPECTS(source[k].get().type() == target.column(k).type(), "Type mismatch in scalar and target column", cudf::data_type_error);
    detail::gx_type(target.column(k).type());
  }
  // every scalar is checked before the first one's validity is read
  std::vector<detail::source> srcs;
  for (auto const& s : source) srcs.push_back(detail::source_of(s.get()));
  detail::result_table out{target.num_columns(), stream, mr};
  auto const* map = static_cast<int32_t const*>(detail::row0(indices));
  for (size_type k = 0; k < target.num_columns(); ++k) {
    srcs[k].may_be_null = detail::scalar_may_be_null(source[k].get(), indices.size() > 0, stream);
    scatter_column(out, srcs[k], map, indices.size(), target.column(k), stream, mr);
  }
  return out.finish(target.num_rows(), true);
}

// ------------------------------------------------------------------------------------ copy_if_else
std::unique_ptr<column> copy_if_else(column_view const& lhs, column_view const& rhs, column_view const& boolean_mask,
                                     rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  check_select(lhs.type(), rhs.type(), boolean_mask);
  CUDF_EXPECTS(lhs.size() == rhs.size(), "Both columns must be of the same size", std::invalid_argument);
  CUDF_EXPECTS(boolean_mask.size() == lhs.size(), "Boolean mask column must be the same size as lhs and rhs columns", std::invalid_argument);
  return select(detail::source_of(lhs), detail::source_of(rhs), boolean_mask, stream, mr);
}

std::unique_ptr<column> copy_if_else(scalar const& lhs, column_view const& rhs, column_view const& boolean_mask,
                                     rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  check_select(lhs.type(), rhs.type(), boolean_mask);
  CUDF_EXPECTS(boolean_mask.size() == rhs.size(), "Boolean mask column must be the same size as rhs column", std::invalid_argument);
  return select(checked_source_of(lhs, boolean_mask.size() > 0, stream), detail::source_of(rhs), boolean_mask, stream, mr);
}

std::unique_ptr<column> copy_if_else(column_view const& lhs, scalar const& rhs, column_view const& boolean_mask,
                                     rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  check_select(lhs.type(), rhs.type(), boolean_mask);
  CUDF_EXPECTS(boolean_mask.size() == lhs.size(), "Boolean mask column must be the same size as lhs column", std::invalid_argument);
  return select(detail::source_of(lhs), checked_source_of(rhs, boolean_mask.size() > 0, stream), boolean_mask, stream, mr);
}

std::unique_ptr<column> copy_if_else(scalar const& lhs, scalar const& rhs, column_view const& boolean_mask,
                                     rmm::cuda_stream_view stream, rmm::device_async_resource_ref mr)
{
  check_select(lhs.type(), rhs.type(), boolean_mask);
  bool const rows = boolean_mask.size() > 0;
  return select(checked_source_of(lhs, rows, stream), checked_source_of(rhs, rows, stream), boolean_mask, stream, mr);
}

// ------------------------------------------------------------------------------------ slice / split
std::vector<column_view> slice(column_view const& input, host_span<size_type const> indices, rmm::cuda_stream_view stream)
{
  check_slice_indices(input.size(), indices);
  std::vector<column_view> out;
  out.reserve(indices.size() / 2);
  for (std::size_t i = 0; i < indices.size(); i += 2) {
    auto const begin = indices[i], end = indices[i + 1];
    auto const nulls = input.has_nulls() ? input.null_count(begin, end, stream) : 0;
    out.emplace_back(input.type(), end - begin, input.head<void>(), input.null_mask(), nulls, input.offset() + begin);
  }
  return out;
}

std::vector<column_view> slice(column_view const& input, std::initializer_list<size_type> indices, rmm::cuda_stream_view stream)
{
  return slice(input, host_span<size_type const>{indices.begin(), indices.size()}, stream);
}

std::vector<table_view> slice(table_view const& input, host_span<size_type const> indices, rmm::cuda_stream_view stream)
{
  check_slice_indices(input.num_rows(), indices);
  std::vector<std::vector<column_view>> pieces(indices.size() / 2);
  for (auto const& c : input) {
    auto const parts = slice(c, indices, stream);
    for (std::size_t p = 0; p < parts.size(); ++p) pieces[p].push_back(parts[p]);
  }
  std::vector<table_view> out;
  out.reserve(pieces.size());
  for (auto const& p : pieces) out.emplace_back(p);
  return out;
}

std::vector<table_view> slice(table_view const& input, std::initializer_list<size_type> indices, rmm::cuda_stream_view stream)
{
  return slice(input, host_span<size_type const>{indices.begin(), indices.size()}, stream);
}

std::vector<column_view> split(column_view const& input, host_span<size_type const> splits, rmm::cuda_stream_view stream)
{
  auto const indices = split_to_slice_indices(input.size(), splits);
  return slice(input, host_span<size_type const>{indices}, stream);
}

std::vector<column_view> split(column_view const& input, std::initializer_list<size_type> splits, rmm::cuda_stream_view stream)
{
  return split(input, host_span<size_type const>{splits.begin(), splits.size()}, stream);
}

std::vector<table_view> split(table_view const& input, host_span<size_type const> splits, rmm::cuda_stream_view stream)
{
  auto const indices = split_to_slice_indices(input.num_rows(), splits);
  return slice(input, host_span<size_type const>{indices}, stream);
}

std::vector<table_view> split(table_view const& input, std::initializer_list<size_type> splits, rmm::cuda_stream_view stream)
{
  return split(input, host_span<size_type const>{splits.begin(), splits.size()}, stream);
}

}  // namespace cudf
