// cudf/copying.hpp -- gather, scatter, copy_if_else, slice and split (reference: cpp/include/cudf/copying.hpp:48-95 for gather;
// kernels cpp/include/cudf/detail/gather.cuh:108-131,506-577; scatter: detail/scatter.cuh, copy_if_else: detail/copy_if_else.cuh,
// slice / split: cpp/src/copying/slice.cu, split.cpp).  cudf::concatenate lives in <cudf/concatenate.hpp>.
#pragma once
#include <cudf/column/column.hpp>
#include <cudf/scalar/scalar.hpp>
#include <cudf/table/table.hpp>
#include <cudf/table/table_view.hpp>
#include <cudf/utilities/span.hpp>

#include <functional>
#include <initializer_list>
#include <memory>
#include <vector>

namespace cudf {

enum class out_of_bounds_policy : bool { NULLIFY, DONT_CHECK };

// out[i] = source_table[gather_map[i]] for every column.  gather_map must be a non-nullable
// INT32 column (the type of join / sorted_order outputs).  NULLIFY: rows whose index is outside
// [0, num_rows) -- e.g. JoinNoMatch -- become null.
std::unique_ptr<table> gather(table_view const& source_table, column_view const& gather_map,
                              out_of_bounds_policy bounds_policy = out_of_bounds_policy::DONT_CHECK,
                              rmm::cuda_stream_view stream       = cudf::get_default_stream(),
                              rmm::device_async_resource_ref mr  = cudf::get_current_device_resource_ref());

// A copy of `target` with target[scatter_map[i]] = source[i] for every column and every i in [0, scatter_map.size()); a negative
// index m means m + target.num_rows().  Indices outside [-n, n) are undefined behaviour: they are not checked.  scatter_map must be
// a non-nullable INT32 column, as gather's map is (a map of another integer type throws cudf::data_type_error where the reference
// takes it; a nullable map throws std::invalid_argument).  A map that repeats a row leaves it with one of its candidates.
// A result column has a null mask only if its target column or its source column has nulls.
// cudf::logic_error: the column counts differ, scatter_map.size() > source.num_rows(); cudf::data_type_error: a source column's
// type differs from its target column's.
std::unique_ptr<table> scatter(table_view const& source, column_view const& scatter_map, table_view const& target,
                               rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                               rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

// The same with one scalar per column: target[indices[i]] = source[column] for every i.  An invalid scalar writes nulls.
// cudf::logic_error: source.size() != target.num_columns(); cudf::data_type_error: a scalar's type differs from its column's.
std::unique_ptr<table> scatter(std::vector<std::reference_wrapper<scalar const>> const& source, column_view const& indices,
                               table_view const& target, rmm::cuda_stream_view stream = cudf::get_default_stream(),
                               rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

// out[i] = boolean_mask[i] is valid and true ? lhs[i] : rhs[i]; a null mask element selects rhs.  The validity of out[i] is the
// chosen side's; the result has a null mask only if a side has nulls (a column) or is invalid (a scalar).  A scalar stands for a
// column of boolean_mask.size() equal rows; with two scalars the size of the result is the mask's.  An empty mask gives an empty
// column.  cudf::data_type_error: boolean_mask is not BOOL8, lhs and rhs differ in type; std::invalid_argument: a column whose
// size is not boolean_mask.size().
std::unique_ptr<column> copy_if_else(column_view const& lhs, column_view const& rhs, column_view const& boolean_mask,
                                     rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                     rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());
std::unique_ptr<column> copy_if_else(scalar const& lhs, column_view const& rhs, column_view const& boolean_mask,
                                     rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                     rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());
std::unique_ptr<column> copy_if_else(column_view const& lhs, scalar const& rhs, column_view const& boolean_mask,
                                     rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                     rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());
std::unique_ptr<column> copy_if_else(scalar const& lhs, scalar const& rhs, column_view const& boolean_mask,
                                     rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                     rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

// Views of the rows [indices[2k], indices[2k + 1]) of `input`, one per pair: no copy, the views share the input's buffers
// (offset + size).  The null count of a piece is counted on the device when the input has nulls (that synchronises `stream`).
// std::invalid_argument: an odd number of indices, begin > end; std::out_of_range: an index outside [0, input.size()].
std::vector<column_view> slice(column_view const& input, host_span<size_type const> indices,
                               rmm::cuda_stream_view stream = cudf::get_default_stream());
std::vector<column_view> slice(column_view const& input, std::initializer_list<size_type> indices,
                               rmm::cuda_stream_view stream = cudf::get_default_stream());
std::vector<table_view> slice(table_view const& input, host_span<size_type const> indices,
                              rmm::cuda_stream_view stream = cudf::get_default_stream());
std::vector<table_view> slice(table_view const& input, std::initializer_list<size_type> indices,
                              rmm::cuda_stream_view stream = cudf::get_default_stream());

// The splits.size() + 1 pieces [0, s0), [s0, s1), ..., [s_last, size): slice on {0, s0, s0, s1, ..., size}, with its throws.
std::vector<column_view> split(column_view const& input, host_span<size_type const> splits,
                               rmm::cuda_stream_view stream = cudf::get_default_stream());
std::vector<column_view> split(column_view const& input, std::initializer_list<size_type> splits,
                               rmm::cuda_stream_view stream = cudf::get_default_stream());
std::vector<table_view> split(table_view const& input, host_span<size_type const> splits,
                              rmm::cuda_stream_view stream = cudf::get_default_stream());
std::vector<table_view> split(table_view const& input, std::initializer_list<size_type> splits,
                              rmm::cuda_stream_view stream = cudf::get_default_stream());

}  // namespace cudf
