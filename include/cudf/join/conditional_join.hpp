// cudf/join/conditional_join.hpp -- joins on an AST predicate over row pairs, returning gather maps
// (reference: cpp/include/cudf/join/conditional_join.hpp; impl cpp/src/join/conditional_join.cu, conditional_join_kernels.cuh).
// `binary_predicate` is a cudf::ast expression whose column references name table_reference::LEFT or table_reference::RIGHT and
// whose result is BOOL8; a pair of rows matches when the predicate is valid and true (a null result is no match).
// The order of the result is fixed here (the reference leaves it open): pairs ascending by (left row, right row); an unmatched
// left row of a left / full join keeps its place as (i, JoinNoMatch); the unmatched right rows of a full join follow as
// (JoinNoMatch, r), r ascending; semi / anti joins return the left rows ascending.
// output_size: accepted as in the reference; the size pass runs anyway (its per-row offsets give the order), and a value that
// disagrees with it throws std::invalid_argument.
// Throws: cudf::data_type_error for a predicate that is not BOOL8 (or has a type error); std::out_of_range for a column index out
// of range of its table; std::invalid_argument beyond the evaluator's limits (32 nodes, 16 columns over both tables, 16 literals,
// 4 spill slots); std::overflow_error for a result of more than 2^31 - 1 rows.
#pragma once
#include <cudf/ast/expressions.hpp>
#include <cudf/join/join.hpp>
#include <cudf/table/table_view.hpp>
#include <cudf/types.hpp>
#include <cudf/utilities/default_stream.hpp>
#include <cudf/utilities/memory_resource.hpp>
#include <rmm/device_uvector.hpp>

#include <cstddef>
#include <memory>
#include <optional>
#include <utility>

namespace cudf {

join_result conditional_inner_join(table_view const& left, table_view const& right, ast::expression const& binary_predicate,
                                   std::optional<std::size_t> output_size = {},
                                   rmm::cuda_stream_view stream           = cudf::get_default_stream(),
                                   rmm::device_async_resource_ref mr      = cudf::get_current_device_resource_ref());

join_result conditional_left_join(table_view const& left, table_view const& right, ast::expression const& binary_predicate,
                                  std::optional<std::size_t> output_size = {},
                                  rmm::cuda_stream_view stream           = cudf::get_default_stream(),
                                  rmm::device_async_resource_ref mr      = cudf::get_current_device_resource_ref());

join_result conditional_full_join(table_view const& left, table_view const& right, ast::expression const& binary_predicate,
                                  rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                  rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

std::unique_ptr<rmm::device_uvector<size_type>> conditional_left_semi_join(
  table_view const& left, table_view const& right, ast::expression const& binary_predicate, std::optional<std::size_t> output_size = {},
  rmm::cuda_stream_view stream = cudf::get_default_stream(), rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

std::unique_ptr<rmm::device_uvector<size_type>> conditional_left_anti_join(
  table_view const& left, table_view const& right, ast::expression const& binary_predicate, std::optional<std::size_t> output_size = {},
  rmm::cuda_stream_view stream = cudf::get_default_stream(), rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

// the rows the join of that name returns: the size pass alone, exact beyond 2^31 - 1
std::size_t conditional_inner_join_size(table_view const& left, table_view const& right, ast::expression const& binary_predicate,
                                        rmm::cuda_stream_view stream = cudf::get_default_stream());
std::size_t conditional_left_join_size(table_view const& left, table_view const& right, ast::expression const& binary_predicate,
                                       rmm::cuda_stream_view stream = cudf::get_default_stream());
std::size_t conditional_left_semi_join_size(table_view const& left, table_view const& right, ast::expression const& binary_predicate,
                                            rmm::cuda_stream_view stream = cudf::get_default_stream());
std::size_t conditional_left_anti_join_size(table_view const& left, table_view const& right, ast::expression const& binary_predicate,
                                            rmm::cuda_stream_view stream = cudf::get_default_stream());

}  // namespace cudf
