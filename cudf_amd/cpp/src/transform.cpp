// cudf::compute_column over the C ABI (gx_compute_column; cudf_amd/csrc/gx_expression.hip).
// reference: cpp/include/cudf/transform.hpp, cpp/src/transform/compute_column.cu, cpp/src/ast/expression_parser.cpp (the
// linearisation of the expression into device data references and operators).  Here the expression is flattened into the post-order
// node array of the kernel layer -- an object under several parents becomes one node -- and one launch writes values, validity words
// and the null count; sliced views are read in place (offset data pointer, begin bit), as binaryop.cpp does.  A mask is allocated
// only when a column the expression reads is nullable or a literal is invalid, and kept only when a row is null: the one host read.
#include "ast_lowering.hpp"
#include "result_column.hpp"

#include <cudf/transform.hpp>

#include <stdexcept>

namespace cudf {
namespace detail {

int32_t flatten_expression(ast::expression const& e, table_view const& left, table_view const* right, rmm::cuda_stream_view stream,
                           flat_expression& f)
{
  if (auto it = f.seen.find(&e); it != f.seen.end()) return it->second;
  gx_expr_node node{0, 0, 0, 0};
  switch (e.kind()) {
    case ast::expression_kind::COLUMN_REFERENCE: {
      auto const& ref  = static_cast<ast::column_reference const&>(e);
      auto const source = ref.get_table_source();
      if (right == nullptr) {
        CUDF_EXPECTS(source == ast::table_reference::LEFT, "Only table_reference::LEFT is evaluated by compute_column", std::invalid_argument);
      } else {
        CUDF_EXPECTS(source == ast::table_reference::LEFT || source == ast::table_reference::RIGHT,
                     "A join predicate reads table_reference::LEFT and table_reference::RIGHT", std::invalid_argument);
      }
      int32_t const side = source == ast::table_reference::RIGHT ? 1 : 0;
      auto const& table  = side ? *right : left;
      auto const idx     = ref.get_column_index();
      CUDF_EXPECTS(idx >= 0 && idx < table.num_columns(), "Column reference is out of range of the table", std::out_of_range);
      int32_t k = 0;
      while (k < static_cast<int32_t>(f.col_index.size()) && (f.col_index[k] != idx || f.cols[k].table != side)) ++k;
      if (k == static_cast<int32_t>(f.col_index.size())) {
        auto const& c = table.column(idx);
        f.col_index.push_back(idx);
        f.col_dtypes.push_back(detail::gx_type(c.type()));
        f.cols.push_back(gx_expr_column{detail::row0(c), c.has_nulls() ? c.null_mask() : nullptr, c.offset(), f.col_dtypes.back(), side});
        f.may_be_null = f.may_be_null || c.has_nulls();
      }
      node = gx_expr_node{GX_EXPR_COLUMN, 0, k, 0};
      break;
    }
    case ast::expression_kind::LITERAL: {
      auto const& lit = static_cast<ast::literal const&>(e);
      auto const& s   = lit.get_value();
      auto const* value = scalar_device_value(s);
      f.lit_dtypes.push_back(detail::gx_type(s.type()));
      f.lits.push_back(gx_expr_literal{value, reinterpret_cast<uint8_t const*>(s.validity_data()), f.lit_dtypes.back(), 0});
      if (right == nullptr && left.num_rows() > 0) f.may_be_null = f.may_be_null || !s.is_valid(stream);  // a join asks for no mask
      node = gx_expr_node{GX_EXPR_LITERAL, 0, static_cast<int32_t>(f.lits.size()) - 1, 0};
      break;
    }
    default: {
      auto const& op = static_cast<ast::operation const&>(e);
      auto const lhs = flatten_expression(op.lhs(), left, right, stream, f);
      auto const rhs = op.is_binary() ? flatten_expression(op.rhs(), left, right, stream, f) : 0;
      node           = gx_expr_node{op.is_binary() ? GX_EXPR_BINARY : GX_EXPR_UNARY, static_cast<int32_t>(op.get_operator()), lhs, rhs};
      break;
    }
  }
  f.nodes.push_back(node);
  auto const index = static_cast<int32_t>(f.nodes.size()) - 1;
  f.seen.emplace(&e, index);
  return index;
}

int expression_result_type(flat_expression const& f)
{
  int max_nodes = 0, max_cols = 0, max_lits = 0;
  gx_expr_limits(&max_nodes, &max_cols, &max_lits, nullptr);
  CUDF_EXPECTS(static_cast<int>(f.nodes.size()) <= max_nodes && static_cast<int>(f.cols.size()) <= max_cols &&
                 static_cast<int>(f.lits.size()) <= max_lits,
               "The expression is beyond the limits of the evaluator", std::invalid_argument);
  int const rc = gx_expr_result_dtype(f.nodes.data(), static_cast<int>(f.nodes.size()), f.col_dtypes.data(), static_cast<int>(f.cols.size()),
                                      f.lit_dtypes.data(), static_cast<int>(f.lits.size()));
  CUDF_EXPECTS(rc != GX_EDTYPE, "The expression has a type error: operands of different types, or an operator that does not take the type",
               cudf::data_type_error);
  CUDF_EXPECTS(rc > 0, "The expression is beyond the limits of the evaluator", std::invalid_argument);  // spill slots, instructions
  return rc;
}

}  // namespace detail

std::unique_ptr<column> compute_column(table_view const& table, ast::expression const& expr, rmm::cuda_stream_view stream,
                                       rmm::device_async_resource_ref mr)
{
  detail::flat_expression f;
  detail::flatten_expression(expr, table, nullptr, stream, f);
  int const rc = detail::expression_result_type(f);
  data_type const output_type{static_cast<type_id>(rc)};
  auto const n = table.num_rows();
  if (n == 0) return make_empty_column(output_type);
  detail::result_column out{output_type, n, f.may_be_null, mask_state::UNINITIALIZED, stream, mr};
  detail::gx_check(gx_compute_column(f.nodes.data(), static_cast<int>(f.nodes.size()), f.cols.data(), static_cast<int>(f.cols.size()),
                                     f.lits.data(), static_cast<int>(f.lits.size()), n, rc, out.data(), out.valid(), out.nulls_dev(),
                                     detail::gxs(stream)),
                   "gx_compute_column");
  return out.finish();
}

}  // namespace cudf
