// cudf/stream_compaction.hpp -- row filtering: cudf::apply_boolean_mask / drop_nulls / drop_nans (reference:
// cpp/include/cudf/stream_compaction.hpp, apply_boolean_mask / drop_nulls / drop_nans; impl
// cpp/src/stream_compaction/apply_boolean_mask.cu, drop_nulls.cu, drop_nans.cu over detail/copy_if.cuh).
// The outputs keep the input's row order and column types; an output column that holds no null comes back without a mask.
// distinct / unique / distinct_count are not on this path.
#pragma once
#include <cudf/column/column_view.hpp>
#include <cudf/table/table.hpp>
#include <cudf/table/table_view.hpp>
#include <cudf/types.hpp>
#include <cudf/utilities/default_stream.hpp>
#include <cudf/utilities/memory_resource.hpp>

#include <memory>
#include <vector>

namespace cudf {

// The rows of `input` with at least keep_threshold valid elements among the columns `keys` (indices into `input`; an index out
// of range throws std::out_of_range, as table_view::select).  No keys, no rows, or keys without any null: a copy of `input`.
// At most 32 key columns (std::invalid_argument beyond).
std::unique_ptr<table> drop_nulls(table_view const& input, std::vector<size_type> const& keys, size_type keep_threshold,
                                  rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                  rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

// keep_threshold = keys.size(): a row with a null in any key column is dropped
std::unique_ptr<table> drop_nulls(table_view const& input, std::vector<size_type> const& keys,
                                  rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                  rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

// The rows of `input` with at least keep_threshold non-NaN elements among the key columns, which must be FLOAT32 / FLOAT64
// (cudf::logic_error otherwise).  A null element is not a NaN.
std::unique_ptr<table> drop_nans(table_view const& input, std::vector<size_type> const& keys, size_type keep_threshold,
                                 rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                 rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

std::unique_ptr<table> drop_nans(table_view const& input, std::vector<size_type> const& keys,
                                 rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                 rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

// The rows i of `input` for which boolean_mask[i] is valid and true.  boolean_mask: BOOL8 (cudf::logic_error otherwise) with as
// many rows as `input` (cudf::logic_error otherwise); a null mask element drops its row.
std::unique_ptr<table> apply_boolean_mask(table_view const& input, column_view const& boolean_mask,
                                          rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                          rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

}  // namespace cudf
