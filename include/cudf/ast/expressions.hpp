// cudf/ast/expressions.hpp -- expression trees for cudf::compute_column (reference: cpp/include/cudf/ast/expressions.hpp).
// An expression is a literal, a column reference or an operation over expressions; nodes refer to each other, so every node has to
// outlive the tree that uses it -- ast::tree owns its nodes for that.  Evaluated by one fused kernel (cudf_amd/csrc/gx_expression.hip):
// the type rules, and which operators are built, are written down in include/cudf_amd/gx.h beside gx_compute_column.
#pragma once
#include <cudf/scalar/scalar.hpp>
#include <cudf/types.hpp>
#include <cudf/utilities/error.hpp>

#include <cstdint>
#include <deque>
#include <memory>
#include <type_traits>
#include <utility>

namespace cudf {
namespace ast {

// the reference's enumerators in the reference's order.  The transcendental operators and CBRT are not built: compute_column throws
// cudf::data_type_error for them.
enum class ast_operator : int32_t {
  // binary
  ADD, SUB, MUL, DIV, TRUE_DIV, FLOOR_DIV, MOD, PYMOD, POW, EQUAL, NULL_EQUAL, NOT_EQUAL, LESS, GREATER, LESS_EQUAL, GREATER_EQUAL,
  BITWISE_AND, BITWISE_OR, BITWISE_XOR, LOGICAL_AND, NULL_LOGICAL_AND, LOGICAL_OR, NULL_LOGICAL_OR,
  // unary
  IDENTITY, IS_NULL, SIN, COS, TAN, ARCSIN, ARCCOS, ARCTAN, SINH, COSH, TANH, ARCSINH, ARCCOSH, ARCTANH, EXP, LOG, SQRT, CBRT, CEIL,
  FLOOR, ABS, RINT, BIT_INVERT, NOT, CAST_TO_INT64, CAST_TO_UINT64, CAST_TO_FLOAT64
};

// which table a column reference reads: compute_column evaluates LEFT only; the conditional joins (join/conditional_join.hpp) LEFT and RIGHT
enum class table_reference { LEFT, RIGHT, OUTPUT };

enum class expression_kind { LITERAL, COLUMN_REFERENCE, OPERATION };

struct expression {
  virtual ~expression() = default;
  [[nodiscard]] virtual expression_kind kind() const noexcept = 0;
};

// a fixed-width scalar in device memory; the scalar has to outlive the evaluation
class literal : public expression {
 public:
  template <typename T>
  literal(cudf::numeric_scalar<T>& value) : _scalar{value}
  {
  }
  [[nodiscard]] expression_kind kind() const noexcept override { return expression_kind::LITERAL; }
  [[nodiscard]] cudf::data_type get_data_type() const { return _scalar.type(); }
  [[nodiscard]] cudf::scalar const& get_value() const { return _scalar; }
  [[nodiscard]] bool is_valid(rmm::cuda_stream_view stream = cudf::get_default_stream()) const { return _scalar.is_valid(stream); }

 private:
  cudf::scalar const& _scalar;
};

class column_reference : public expression {
 public:
  column_reference(cudf::size_type column_index, table_reference table_source = table_reference::LEFT)
    : _column_index{column_index}, _table_source{table_source}
  {
  }
  [[nodiscard]] expression_kind kind() const noexcept override { return expression_kind::COLUMN_REFERENCE; }
  [[nodiscard]] cudf::size_type get_column_index() const { return _column_index; }
  [[nodiscard]] table_reference get_table_source() const { return _table_source; }

 private:
  cudf::size_type _column_index;
  table_reference _table_source;
};

class operation : public expression {
 public:
  // std::invalid_argument when the operator does not take that many operands
  operation(ast_operator op, expression const& input) : _op{op}, _lhs{&input}, _rhs{nullptr}
  {
    CUDF_EXPECTS(op >= ast_operator::IDENTITY, "The provided operator is not a unary operator.", std::invalid_argument);
  }
  operation(ast_operator op, expression const& left, expression const& right) : _op{op}, _lhs{&left}, _rhs{&right}
  {
    CUDF_EXPECTS(op < ast_operator::IDENTITY, "The provided operator is not a binary operator.", std::invalid_argument);
  }
  // a temporary operand would dangle
  operation(ast_operator, expression&&)                      = delete;
  operation(ast_operator, expression&&, expression&&)        = delete;
  operation(ast_operator, expression const&, expression&&)   = delete;
  operation(ast_operator, expression&&, expression const&)   = delete;

  [[nodiscard]] expression_kind kind() const noexcept override { return expression_kind::OPERATION; }
  [[nodiscard]] ast_operator get_operator() const { return _op; }
  [[nodiscard]] bool is_binary() const { return _rhs != nullptr; }
  [[nodiscard]] expression const& lhs() const { return *_lhs; }
  [[nodiscard]] expression const& rhs() const { return *_rhs; }

 private:
  ast_operator _op;
  expression const* _lhs;
  expression const* _rhs;
};

// owns the nodes of an expression, so that a function can build and return one: the addresses of the nodes are stable
class tree {
 public:
  tree()                       = default;
  tree(tree&&)                 = default;
  tree& operator=(tree&&)      = default;
  tree(tree const&)            = delete;
  tree& operator=(tree const&) = delete;

  template <typename Expr, typename... Args>
  std::enable_if_t<std::is_base_of_v<expression, Expr>, Expr const&> emplace(Args&&... args)
  {
    auto node       = std::make_unique<Expr>(std::forward<Args>(args)...);
    Expr const& ref = *node;
    _nodes.emplace_back(std::move(node));
    return ref;
  }
  template <typename Expr>
  std::enable_if_t<std::is_base_of_v<expression, std::decay_t<Expr>>, std::decay_t<Expr> const&> push(Expr&& expr)
  {
    return emplace<std::decay_t<Expr>>(std::forward<Expr>(expr));
  }
  [[nodiscard]] expression const& front() const { return *_nodes.front(); }
  [[nodiscard]] expression const& back() const { return *_nodes.back(); }  // the node added last: by convention the root
  [[nodiscard]] std::size_t size() const { return _nodes.size(); }
  [[nodiscard]] expression const& at(std::size_t index) const { return *_nodes.at(index); }
  [[nodiscard]] expression const& operator[](std::size_t index) const { return *_nodes[index]; }

 private:
  std::deque<std::unique_ptr<expression>> _nodes;
};

}  // namespace ast
}  // namespace cudf
