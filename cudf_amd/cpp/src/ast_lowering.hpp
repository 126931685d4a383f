// ast_lowering.hpp -- cudf::ast expressions as the post-order node array of the kernel layer (gx_expr_node): the one tree walk,
// shared by compute_column (one table) and the conditional joins (two).  Defined in transform.cpp.
#pragma once
#include "common.hpp"

#include <cudf/ast/expressions.hpp>

#include <unordered_map>
#include <vector>

namespace cudf {
namespace detail {

struct flat_expression {
  std::vector<gx_expr_node> nodes;
  std::vector<gx_expr_column> cols;  // the distinct (table, column) pairs the expression reads, in first-use order
  std::vector<gx_expr_literal> lits;
  std::vector<int32_t> col_dtypes, lit_dtypes;
  std::vector<size_type> col_index;  // table column of cols[k]
  std::unordered_map<ast::expression const*, int32_t> seen;
  bool may_be_null{false};
};

// Appends the nodes of `e` to f and returns the index of its root; an object under several parents becomes one node.  right ==
// nullptr: one table, a reference to another one throws std::invalid_argument.  A column index out of range of its table throws
// std::out_of_range; sliced views are read in place (offset data pointer, begin bit).
int32_t flatten_expression(ast::expression const& e, table_view const& left, table_view const* right, rmm::cuda_stream_view stream,
                           flat_expression& f);

// the root's type_id; std::invalid_argument beyond the evaluator's limits, cudf::data_type_error for a type error
int expression_result_type(flat_expression const& f);

}  // namespace detail
}  // namespace cudf
