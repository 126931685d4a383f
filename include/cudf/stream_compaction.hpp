// cudf/stream_compaction.hpp -- row filtering: cudf::apply_boolean_mask / drop_nulls / drop_nans, and deduplication: cudf::unique /
// distinct / stable_distinct / distinct_indices / unique_count / distinct_count (reference: cpp/include/cudf/stream_compaction.hpp;
// impl cpp/src/stream_compaction/apply_boolean_mask.cu, drop_nulls.cu, drop_nans.cu over detail/copy_if.cuh, and unique.cu,
// distinct.cu, stable_distinct.cu, distinct_helpers.cu, unique_count.cu, distinct_count.cu).
// The outputs keep the input's row order and column types; an output column that holds no null comes back without a mask.
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

// ---- deduplication.  Row equality over the key columns: two elements are equal when both are null and nulls_equal == EQUAL, or both
// are valid with equal values; for floats -0.0 == +0.0, and NaN == NaN (any sign, any payload) iff NaNs are equal.  A null and a
// valid element are never equal.  A row that holds a null under null_equality::UNEQUAL (a NaN under nan_equality::UNEQUAL) equals
// no row: it is always kept, under KEEP_NONE as well.  1 .. 32 key columns (std::invalid_argument beyond); an index out of range
// throws std::out_of_range, as table_view::select.  No keys or no rows: a copy of `input`.
enum class duplicate_keep_option {
  KEEP_ANY = 0,  // one row of every set of equal rows, whichever
  KEEP_FIRST,    // the first (smallest row index)
  KEEP_LAST,     // the last
  KEEP_NONE      // only the rows that have no duplicate
};

// Collapses runs of CONSECUTIVE equal rows; row order is kept; NaNs compare equal.  KEEP_FIRST / KEEP_ANY keep the first row of a
// run, KEEP_LAST the last, KEEP_NONE only the runs of length 1.
std::unique_ptr<table> unique(table_view const& input, std::vector<size_type> const& keys, duplicate_keep_option keep,
                              null_equality nulls_equal         = null_equality::EQUAL,
                              rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                              rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

// One row per set of equal rows of the whole table.  The reference leaves the output order unspecified; here it is the input's
// row order, always (distinct IS stable_distinct).
std::unique_ptr<table> distinct(table_view const& input, std::vector<size_type> const& keys,
                                duplicate_keep_option keep        = duplicate_keep_option::KEEP_ANY,
                                null_equality nulls_equal         = null_equality::EQUAL,
                                nan_equality nans_equal           = nan_equality::ALL_EQUAL,
                                rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

std::unique_ptr<table> stable_distinct(table_view const& input, std::vector<size_type> const& keys,
                                       duplicate_keep_option keep        = duplicate_keep_option::KEEP_ANY,
                                       null_equality nulls_equal         = null_equality::EQUAL,
                                       nan_equality nans_equal           = nan_equality::ALL_EQUAL,
                                       rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                       rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

// INT32 column of the row indices distinct() keeps when every column of `input` is a key, in ascending order.
std::unique_ptr<column> distinct_indices(table_view const& input, duplicate_keep_option keep = duplicate_keep_option::KEEP_ANY,
                                         null_equality nulls_equal         = null_equality::EQUAL,
                                         nan_equality nans_equal           = nan_equality::ALL_EQUAL,
                                         rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                         rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

// Number of rows unique() / distinct() would keep under KEEP_ANY (NaNs equal); nothing is compacted.  0 for no rows.
size_type unique_count(table_view const& input, null_equality nulls_equal = null_equality::EQUAL,
                       rmm::cuda_stream_view stream = cudf::get_default_stream());
size_type distinct_count(table_view const& input, null_equality nulls_equal = null_equality::EQUAL,
                         rmm::cuda_stream_view stream = cudf::get_default_stream());

// One column under the policy switches: NAN_IS_NULL treats a NaN element as a null element, NAN_IS_VALID all NaNs as one value;
// null_policy::INCLUDE lets the nulls form one value that counts once, EXCLUDE never counts a null row.  unique_count compares a row
// with the physically previous one whether that one counts or not: [1, null, 1] under EXCLUDE is 2.
size_type unique_count(column_view const& input, null_policy null_handling, nan_policy nan_handling,
                       rmm::cuda_stream_view stream = cudf::get_default_stream());
size_type distinct_count(column_view const& input, null_policy null_handling, nan_policy nan_handling,
                         rmm::cuda_stream_view stream = cudf::get_default_stream());

}  // namespace cudf
