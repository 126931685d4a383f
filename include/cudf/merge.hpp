// cudf/merge.hpp -- cudf::merge: sorted tables combined into one sorted table (reference: cpp/include/cudf/merge.hpp; impl
// cpp/src/merge/merge.cu).
// Here the merge is STABLE: rows that compare equivalent come out ordered by (index of their table, row).  The reference leaves the
// order of such rows open, so this is one of the results it allows.
#pragma once
#include <cudf/table/table.hpp>
#include <cudf/table/table_view.hpp>
#include <cudf/types.hpp>
#include <cudf/utilities/default_stream.hpp>
#include <cudf/utilities/memory_resource.hpp>

#include <memory>
#include <vector>

namespace cudf {

// tables_to_merge: tables of the same column types, each sorted on the columns key_cols under column_order / null_precedence (one
// entry per KEY; an empty null_precedence = null_order::BEFORE for every key).  Key columns are fixed-width numerics, at most 32 of
// them; every other column rides along, with any fixed width and validity.  An output column that holds no null comes back without
// a mask.  No tables: an empty table.  One table: a copy.  Tables without rows add nothing.
// cudf::logic_error: no key columns, more keys than columns, column_order not one per key, a non-empty null_precedence of another
// size, tables whose column counts or types differ.  std::out_of_range: a key index outside the table.  std::overflow_error: the
// total row count does not fit size_type.
std::unique_ptr<table> merge(std::vector<table_view> const& tables_to_merge, std::vector<size_type> const& key_cols,
                             std::vector<order> const& column_order, std::vector<null_order> const& null_precedence = {},
                             rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                             rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

}  // namespace cudf
