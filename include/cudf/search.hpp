// cudf/search.hpp -- cudf::lower_bound / upper_bound: insertion points of needle rows in a sorted haystack (reference:
// cpp/include/cudf/search.hpp; impl cpp/src/search/search_ordered.cu).  cudf::contains is not provided.
#pragma once
#include <cudf/column/column.hpp>
#include <cudf/table/table_view.hpp>
#include <cudf/types.hpp>
#include <cudf/utilities/default_stream.hpp>
#include <cudf/utilities/memory_resource.hpp>

#include <memory>
#include <vector>

namespace cudf {

// haystack: sorted under column_order / null_precedence (one entry per column; an empty null_precedence = null_order::BEFORE
// everywhere); needles: rows of the same column types, in any order.  Fixed-width numeric columns, at most 32.
// Result: a non-nullable INT32 column of needles.num_rows(): for needle i the number of haystack rows that compare strictly less
// (lower_bound) or less than or equal (upper_bound) under the lexicographic row comparator -- nulls equivalent, NaNs equivalent
// and greater than every number, -0.0 == +0.0.
// cudf::logic_error: column counts or types of haystack and needles differ, column_order not one per column, a non-empty
// null_precedence of another size.
std::unique_ptr<column> lower_bound(table_view const& haystack, table_view const& needles, std::vector<order> const& column_order,
                                    std::vector<null_order> const& null_precedence,
                                    rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                    rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

std::unique_ptr<column> upper_bound(table_view const& haystack, table_view const& needles, std::vector<order> const& column_order,
                                    std::vector<null_order> const& null_precedence,
                                    rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                    rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

}  // namespace cudf
