"""Expression trees for ops.compute_column (cudf::ast: expressions.hpp).

``ColumnReference(index)``, ``Literal(value, dtype)`` and ``Operation(op, lhs, rhs=None)`` build a tree; operator names are those of
cudf::ast::ast_operator ("ADD", "LESS", "CAST_TO_FLOAT64", ...).  There is no implicit promotion: the operands of a binary operator
must have the same dtype, a caller inserts CAST_TO_* nodes.  ``flatten`` turns a tree into the post-order node array of the C ABI
(include/cudf_amd/gx.h: gx_expr_node); an object that appears under several parents becomes one node with several parents.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import numpy as np

from . import _lib as L


class Expression:
    __slots__ = ()


class ColumnReference(Expression):
    """column `index` of the table `table`: "left" (the one table of compute_column) or "right" (the other side of a conditional join)"""
    __slots__ = ("index", "table")

    def __init__(self, index: int, table: str = "left"):
        if int(index) != index or index < 0:
            raise ValueError(f"column index {index!r} must be a non-negative integer")
        if table not in ("left", "right"):
            raise ValueError(f"table {table!r} must be 'left' or 'right'")
        self.index = int(index)
        self.table = table


class Literal(Expression):
    """a scalar of `dtype`; value None is the invalid (null) literal"""
    __slots__ = ("value", "dtype")

    def __init__(self, value, dtype):
        from .column import gx_dtype
        self.dtype = np.dtype(dtype)
        gx_dtype(self.dtype)                 # TypeError for a dtype the kernels do not take
        if value is not None:
            from .ops import _check_scalar
            _check_scalar(value, self.dtype)  # TypeError when the dtype cannot hold it
        self.value = value


class Operation(Expression):
    __slots__ = ("op", "lhs", "rhs")

    def __init__(self, op, lhs: Expression, rhs: Optional[Expression] = None):
        if isinstance(op, str):
            if op.upper() not in L.AST_OP:
                raise ValueError(f"unknown ast operator {op!r}")
            code = L.AST_OP[op.upper()]
        else:
            code = int(op)
            if not 0 <= code < len(L.AST_OPS):
                raise ValueError(f"unknown ast operator {op!r}")
        unary = code >= L.AST_FIRST_UNARY
        if unary != (rhs is None):
            raise ValueError(f"{L.AST_OPS[code]} takes {'one operand' if unary else 'two operands'}")
        for side in (lhs,) if unary else (lhs, rhs):
            if not isinstance(side, Expression):
                raise TypeError(f"operand {side!r} is not an expression")
        self.op, self.lhs, self.rhs = code, lhs, rhs

    @property
    def name(self) -> str:
        return L.AST_OPS[self.op]


def flatten(expr: Expression) -> Tuple[List[Tuple[int, int, int, int]], List[int], List[Literal]]:
    """(nodes, column indices, literals): nodes are (kind, op, lhs, rhs) in post order, the root last; a COLUMN node's lhs indexes
    `column indices` (the distinct table columns the expression reads, in first-use order), a LITERAL node's lhs `literals`.
    ValueError for a reference to the right table: there is one table here (flatten_pair takes two)"""
    nodes, columns, literals = flatten_pair(expr)
    if any(table == "right" for table, _ in columns):
        raise ValueError("the expression refers to the right table: only a conditional join has one")
    return nodes, [index for _, index in columns], literals


def flatten_pair(expr: Expression) -> Tuple[List[Tuple[int, int, int, int]], List[Tuple[str, int]], List[Literal]]:
    """flatten for a predicate over two tables: the columns are (table, index) pairs, "left" / "right", in first-use order"""
    if not isinstance(expr, Expression):
        raise TypeError(f"{expr!r} is not an expression")
    nodes: List[Tuple[int, int, int, int]] = []
    columns: List[Tuple[str, int]] = []
    literals: List[Literal] = []
    seen = {}

    def visit(e) -> int:
        if id(e) in seen:
            return seen[id(e)]
        if isinstance(e, ColumnReference):
            key = (e.table, e.index)
            if key not in columns:
                columns.append(key)
            node = (L.EXPR_COLUMN, 0, columns.index(key), 0)
        elif isinstance(e, Literal):
            literals.append(e)
            node = (L.EXPR_LITERAL, 0, len(literals) - 1, 0)
        else:
            lhs = visit(e.lhs)
            node = (L.EXPR_UNARY, e.op, lhs, 0) if e.rhs is None else (L.EXPR_BINARY, e.op, lhs, visit(e.rhs))
        nodes.append(node)
        seen[id(e)] = len(nodes) - 1
        return seen[id(e)]

    visit(expr)
    return nodes, columns, literals


# ------------------------------------------------------------------------------------------------ DataFrame.eval / query
_FLOATS = (np.dtype(np.float32), np.dtype(np.float64))
_BOOL = np.dtype(np.bool_)
_BOOL_RESULT = {"EQUAL", "NOT_EQUAL", "LESS", "GREATER", "LESS_EQUAL", "GREATER_EQUAL", "LOGICAL_AND", "LOGICAL_OR", "NULL_EQUAL",
                "NULL_LOGICAL_AND", "NULL_LOGICAL_OR", "NOT", "IS_NULL"}
_CASTS = {"CAST_TO_INT64": np.dtype(np.int64), "CAST_TO_UINT64": np.dtype(np.uint64), "CAST_TO_FLOAT64": np.dtype(np.float64)}


def compute_class(dt) -> np.dtype:
    """C(T): INT32 for bool and everything narrower than 32 bits, else T"""
    dt = np.dtype(dt)
    return np.dtype(np.int32) if dt.itemsize < 4 else dt


def result_dtype(op: str, dt) -> np.dtype:
    """the dtype of `op` on operands of dtype dt under the rules of gx.h (no check that the operator takes the dtype)"""
    dt = np.dtype(dt)
    if op in _BOOL_RESULT:
        return _BOOL
    if op in _CASTS:
        return _CASTS[op]
    if op in ("TRUE_DIV", "FLOOR_DIV"):
        return np.dtype(np.float64)
    if op == "POW":
        return dt if dt == np.float32 else np.dtype(np.float64)
    if op in ("IDENTITY", "SQRT", "CEIL", "FLOOR", "RINT"):
        return dt
    return compute_class(dt)


def common_cast(a, b) -> str:
    """the cast both sides of an eval operator get when their dtypes differ"""
    a, b = np.dtype(a), np.dtype(b)
    if a in _FLOATS or b in _FLOATS:
        return "CAST_TO_FLOAT64"
    return "CAST_TO_UINT64" if a.kind == "u" and b.kind == "u" else "CAST_TO_INT64"


class _Const:
    """a Python literal whose dtype is still open: it takes the dtype of the other side"""
    __slots__ = ("value",)

    def __init__(self, value):
        self.value = value

    def natural(self):
        v = self.value
        return Literal(v, np.bool_ if isinstance(v, bool) else (np.int64 if isinstance(v, int) else np.float64))


def parse_eval(text: str, dtypes: dict, right_dtypes: Optional[dict] = None):
    """The expression of DataFrame.eval: `text` over the columns `dtypes` (name -> dtype, in table order).  Returns (expression,
    dtype).  With right_dtypes (DataFrame.join_where) the expression is over two frames: `left.name` / `right.name` name a column
    of one frame, a bare name must occur in exactly one of them (in both: ValueError).  Grammar: column names, numeric literals, + - * / // % **, the six comparisons, & | ~, and / or / not, parentheses.
    / is TRUE_DIV and // FLOOR_DIV (both FLOAT64), % PYMOD, ** POW; & | ~ are logical on bool operands and bitwise on integers.
    Operands of different dtypes are both cast (common_cast); a literal takes the dtype of the other side (TypeError when that
    dtype cannot hold it).  Anything else is a ValueError that names the construct."""
    import ast as pyast
    names = list(dtypes)
    try:
        tree = pyast.parse(text.strip(), mode="eval")
    except SyntaxError as e:
        raise ValueError(f"eval: cannot parse {text!r}: {e.msg}") from None

    def bad(node, what=None):
        raise ValueError(f"eval: {what or type(node).__name__} is not supported in {text!r}")

    def typed(x):
        """(expression, dtype) of an operand that stands alone"""
        if isinstance(x, _Const):
            lit = x.natural()
            return lit, lit.dtype
        return x

    def unify(l, r):
        if isinstance(l, _Const) and isinstance(r, _Const):
            l, r = typed(l), typed(r)
        if isinstance(l, _Const):
            return (Literal(l.value, r[1]), r[1]), r
        if isinstance(r, _Const):
            return l, (Literal(r.value, l[1]), l[1])
        if l[1] != r[1]:
            cast = common_cast(l[1], r[1])
            return (Operation(cast, l[0]), _CASTS[cast]), (Operation(cast, r[0]), _CASTS[cast])
        return l, r

    def binary(name, l, r, node):
        l, r = unify(l, r)
        dt = l[1]
        if name in ("AND", "OR"):             # & and |
            if dt == _BOOL:
                name = "LOGICAL_" + name
            elif dt.kind in "iu":
                name = "BITWISE_" + name
            else:
                raise TypeError(f"eval: {'&' if name == 'AND' else '|'} is not supported for {dt} in {text!r}")
        return Operation(name, l[0], r[0]), result_dtype(name, dt)

    binops = {pyast.Add: "ADD", pyast.Sub: "SUB", pyast.Mult: "MUL", pyast.Div: "TRUE_DIV", pyast.FloorDiv: "FLOOR_DIV",
              pyast.Mod: "PYMOD", pyast.Pow: "POW", pyast.BitAnd: "AND", pyast.BitOr: "OR"}
    cmps = {pyast.Eq: "EQUAL", pyast.NotEq: "NOT_EQUAL", pyast.Lt: "LESS", pyast.Gt: "GREATER", pyast.LtE: "LESS_EQUAL",
            pyast.GtE: "GREATER_EQUAL"}

    def visit(node):
        if isinstance(node, pyast.Expression):
            return visit(node.body)
        if right_dtypes is not None and isinstance(node, pyast.Attribute) and isinstance(node.value, pyast.Name) \
                and node.value.id in ("left", "right"):
            side = dtypes if node.value.id == "left" else right_dtypes
            if node.attr not in side:
                raise KeyError(f"{node.value.id}.{node.attr}")
            return ColumnReference(list(side).index(node.attr), node.value.id), np.dtype(side[node.attr])
        if isinstance(node, pyast.Name):
            if right_dtypes is not None and node.id in right_dtypes:
                if node.id in dtypes:
                    raise ValueError(f"eval: the name {node.id!r} is in both frames: write left.{node.id} or right.{node.id} in {text!r}")
                return ColumnReference(list(right_dtypes).index(node.id), "right"), np.dtype(right_dtypes[node.id])
            if node.id not in dtypes:
                raise KeyError(node.id)
            return ColumnReference(names.index(node.id)), np.dtype(dtypes[node.id])
        if isinstance(node, pyast.Constant):
            if not isinstance(node.value, (bool, int, float)):
                bad(node, f"the literal {node.value!r}")
            return _Const(node.value)
        if isinstance(node, pyast.BinOp):
            if type(node.op) not in binops:
                bad(node, f"the operator {type(node.op).__name__}")
            return binary(binops[type(node.op)], visit(node.left), visit(node.right), node)
        if isinstance(node, pyast.Compare):
            if len(node.ops) != 1:
                bad(node, "a chained comparison")
            if type(node.ops[0]) not in cmps:
                bad(node, f"the comparison {type(node.ops[0]).__name__}")
            return binary(cmps[type(node.ops[0])], visit(node.left), visit(node.comparators[0]), node)
        if isinstance(node, pyast.BoolOp):
            name = "LOGICAL_AND" if isinstance(node.op, pyast.And) else "LOGICAL_OR"
            acc = visit(node.values[0])
            for v in node.values[1:]:
                acc = binary(name, acc, visit(v), node)
            return acc
        if isinstance(node, pyast.UnaryOp):
            operand = visit(node.operand)
            if isinstance(node.op, (pyast.USub, pyast.UAdd)):
                if isinstance(operand, _Const) and not isinstance(operand.value, bool):
                    return _Const(-operand.value if isinstance(node.op, pyast.USub) else operand.value)
                bad(node, f"unary {'-' if isinstance(node.op, pyast.USub) else '+'} on anything but a numeric literal")
            e, dt = typed(operand)
            if isinstance(node.op, pyast.Not) or dt == _BOOL:
                return Operation("NOT", e), _BOOL
            if dt.kind not in "iu":
                raise TypeError(f"eval: ~ is not supported for {dt} in {text!r}")
            return Operation("BIT_INVERT", e), result_dtype("BIT_INVERT", dt)
        bad(node)

    return typed(visit(tree))
