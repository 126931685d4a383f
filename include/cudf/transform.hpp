// cudf/transform.hpp -- compute_column: one expression tree over the columns of a table (reference: cpp/include/cudf/transform.hpp,
// cpp/src/transform/compute_column.cu).  Kernel: cudf_amd/csrc/gx_expression.hip -- the whole expression is one launch and no
// intermediate column is written.  The other functions of the reference's header are not built.
#pragma once
#include <cudf/ast/expressions.hpp>
#include <cudf/column/column.hpp>
#include <cudf/table/table_view.hpp>

#include <memory>

namespace cudf {

// out[i] = expr over row i of `table` (table_reference::LEFT).  The result type follows the rules beside gx_compute_column in
// include/cudf_amd/gx.h: no implicit promotion -- the operands of a binary operator have the same type, a caller inserts CAST_TO_*.
// A row is null where an operand of a node is (IS_NULL, NULL_EQUAL, NULL_LOGICAL_AND / OR have their own rules); the result has a
// mask only when a column the expression reads is nullable or a literal is invalid.  Sliced views are read in place.
// cudf::data_type_error: operands of different types, an operator that does not take the type or is not built;
// std::out_of_range: a column index outside the table;  std::invalid_argument: an expression beyond the evaluator's limits
// (gx_expr_limits), a reference to another table than LEFT.
std::unique_ptr<column> compute_column(table_view const& table, ast::expression const& expr,
                                       rmm::cuda_stream_view stream      = cudf::get_default_stream(),
                                       rmm::device_async_resource_ref mr = cudf::get_current_device_resource_ref());

}  // namespace cudf
