"""CPU: cudf::compute_column as far as it can be checked without a device -- exported symbols, the argument checks of
gx_compute_column / gx_expr_result_dtype / gx_expr_plan with fake pointers (nothing is launched), gx_expr_limits, the --host cases of
the C++ surface, the plan of gx_expr_plan run in a NumPy interpreter of the accumulator machine against a recursive evaluation of
the tree (tests/expression_model.py), and the parser of DataFrame.eval."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import expression_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cudf_amd", "libcudf.so")
GXLIB = os.path.join(ROOT, "cudf_amd", "libcudf_amd.so")
BIN = os.path.join(ROOT, "tests", "cpp", "cudf_transform_tests")

GX_EINVAL, GX_EDTYPE, GX_EOVERFLOW = -1, -2, -5
NEW = ("gx_compute_column", "gx_expr_result_dtype", "gx_expr_plan", "gx_expr_limits", "gx_expression_tile_rows",
       "gx_expression_grid_cap")


@pytest.fixture(autouse=True, scope="module")
def _the_kernel_layer_has_the_evaluator():
    import __graft_entry__ as ge
    ge.build()
    from cudf_amd import _lib
    assert hasattr(_lib.lib, "gx_compute_column") and "gx_compute_column" in _lib.EXPORTED


# ------------------------------------------------------------------------------------------------ helpers over the C ABI
def _node_array(nodes):
    from cudf_amd import _lib as L
    return (L.ExprNode * max(len(nodes), 1))(*[L.ExprNode(*nd) for nd in nodes])


def _i32(values):
    return (ctypes.c_int32 * max(len(values), 1))(*values)


def result_dtype(nodes, col_dtypes, lit_dtypes=()):
    from cudf_amd import _lib as L
    return L.lib.gx_expr_result_dtype(_node_array(nodes), len(nodes), _i32(col_dtypes), len(col_dtypes), _i32(lit_dtypes), len(lit_dtypes))


def plan(nodes, col_dtypes, lit_dtypes=(), capacity=64):
    """(rc, instruction tuples, n_slots)"""
    from cudf_amd import _lib as L
    ins = (L.ExprInstr * max(capacity, 1))()
    ni, ns = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = L.lib.gx_expr_plan(_node_array(nodes), len(nodes), _i32(col_dtypes), len(col_dtypes), _i32(lit_dtypes), len(lit_dtypes), ins,
                            capacity, ctypes.byref(ni), ctypes.byref(ns))
    got = [(i.kind, i.op, i.src_kind, i.src_index, i.in_dtype, i.out_dtype) for i in ins[:max(min(ni.value, capacity), 0)]]
    return rc, got, ns.value, ni.value


def compute(nodes, cols, lits=(), n=7, out_dtype=None, out=0x30000, out_valid=None):
    """gx_compute_column on fake pointers: cols = [(dtype, data address, begin bit)], lits = [(dtype, value address)]"""
    from cudf_amd import _lib as L
    ca = (L.ExprColumn * max(len(cols), 1))(*[L.ExprColumn(d, None, b, t, 0) for t, d, b in cols])
    la = (L.ExprLiteral * max(len(lits), 1))(*[L.ExprLiteral(v, None, t, 0) for t, v in lits])
    if out_dtype is None:
        out_dtype = result_dtype(nodes, [c[0] for c in cols], [l[0] for l in lits])
    return L.lib.gx_compute_column(_node_array(nodes), len(nodes), ca, len(cols), la, len(lits), n, out_dtype,
                                   ctypes.c_void_p(out) if out else None, out_valid, None, None)


C0, C1, L0 = (M.COLUMN, 0, 0, 0), (M.COLUMN, 0, 1, 0), (M.LITERAL, 0, 0, 0)


def B(op, lhs, rhs):
    return (M.BINARY, M.OP[op], lhs, rhs)


def U(op, child):
    return (M.UNARY, M.OP[op], child, 0)


# ------------------------------------------------------------------------------------------------ symbols, limits
def test_libraries_export_the_expression_api():
    from cudf_amd import _lib
    defined = subprocess.check_output(["nm", "-D", "--defined-only", GXLIB], text=True)
    for s in NEW:
        assert s in _lib.EXPORTED and hasattr(_lib.lib, s) and f" T {s}\n" in defined
    # the new source pulls in nothing the library did not need before: no undefined symbol of the kernel layer itself
    und = subprocess.check_output(["nm", "-D", "--undefined-only", GXLIB], text=True)
    assert not [l for l in und.splitlines() if " gx_" in l or "_ZN2gx" in l], und
    syms = subprocess.check_output(["nm", "-DC", "--defined-only", LIB], text=True)
    assert syms.count("cudf::compute_column(") == 1
    assert "gx_compute_column" in subprocess.check_output(["nm", "-D", "--undefined-only", LIB], text=True)
    for h in ("transform.hpp", os.path.join("ast", "expressions.hpp")):
        assert os.path.exists(os.path.join(ROOT, "include", "cudf", h))


def test_operator_codes_mirror_the_header():
    import re
    from cudf_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "cudf_amd", "gx.h")).read()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"GX_AST_([A-Z0-9_]+) = (\d+)", text)}
    assert codes == L.AST_OP == M.OP and len(codes) == 50
    assert L.AST_FIRST_UNARY == 23 and L.AST_OPS[22] == "NULL_LOGICAL_OR"


def test_limits_and_tile_rows():
    from cudf_amd import _lib as L
    v = [ctypes.c_int(0) for _ in range(4)]
    L.lib.gx_expr_limits(*[ctypes.byref(x) for x in v])
    nodes, cols, lits, slots = (x.value for x in v)
    assert nodes >= 32 and cols >= 16 and lits >= 16 and slots >= 4
    L.lib.gx_expr_limits(None, None, None, None)                 # every output is optional
    T = L.lib.gx_expression_tile_rows()
    assert T > 0 and T % 32 == 0                                 # a tile owns whole validity words
    assert L.lib.gx_expression_grid_cap() > 0
    # one past each limit is GX_EINVAL from every entry point, never a truncated program
    chain = [C0] + [U("IDENTITY", i) for i in range(nodes)]      # nodes + 1 nodes
    assert result_dtype(chain, [M.INT32]) == GX_EINVAL and plan(chain, [M.INT32])[0] == GX_EINVAL
    assert compute(chain, [(M.INT32, 0x10000, 0)], out_dtype=M.INT32) == GX_EINVAL
    assert result_dtype(chain[:nodes], [M.INT32]) == M.INT32
    assert result_dtype([C0], [M.INT32] * (cols + 1)) == GX_EINVAL and result_dtype([C0], [M.INT32] * cols) == M.INT32
    assert result_dtype([C0], [M.INT32], [M.INT32] * (lits + 1)) == GX_EINVAL
    assert compute([C0], [(M.INT32, 0x10000, 0)] * (cols + 1), out_dtype=M.INT32) == GX_EINVAL


def _spill_tree(depth):
    """a node array whose root needs `depth` spill slots: every level joins two copies of the level below (one shared node)"""
    nodes = [C0, U("ABS", 0)]
    for _ in range(depth):
        top = len(nodes) - 1
        nodes.append(B("ADD", top, top))
    return nodes


def test_one_slot_more_than_the_limit_is_an_error():
    from cudf_amd import _lib as L
    slots = ctypes.c_int(0)
    L.lib.gx_expr_limits(None, None, None, ctypes.byref(slots))
    rc, ins, ns, ni = plan(_spill_tree(slots.value), [M.INT64])
    assert rc == 0 and ns == slots.value and {i[3] for i in ins if i[0] == M.SPILL} == set(range(slots.value))
    assert M.expansion(_spill_tree(slots.value))[:2] == (ni, ns)
    deeper = _spill_tree(slots.value + 1)
    assert plan(deeper, [M.INT64])[0] == GX_EINVAL and result_dtype(deeper, [M.INT64]) == GX_EINVAL
    assert compute(deeper, [(M.INT64, 0x10000, 0)], out_dtype=M.INT64) == GX_EINVAL


# ------------------------------------------------------------------------------------------------ argument checks
def test_malformed_node_arrays_are_einval_before_any_device_call():
    i32 = [(M.INT32, 0x10000, 0), (M.INT32, 0x20000, 0)]
    good = [C0, C1, B("ADD", 0, 1)]
    cases = {
        "child not below its parent": [C0, C1, B("ADD", 0, 2)],
        "right child not below its parent": [C0, C1, B("ADD", 3, 1)],
        "negative child": [C0, U("ABS", -1)],
        "unary child is itself": [C0, U("ABS", 1)],
        "column index out of range": [C0, (M.COLUMN, 0, 2, 0), B("ADD", 0, 1)],
        "negative column index": [(M.COLUMN, 0, -1, 0)],
        "literal index out of range": [C0, (M.LITERAL, 0, 0, 0), B("ADD", 0, 1)],
        "operator outside the enum": [C0, C1, (M.BINARY, 50, 0, 1)],
        "negative operator": [C0, C1, (M.BINARY, -1, 0, 1)],
        "a unary operator on a binary node": [C0, C1, (M.BINARY, M.OP["ABS"], 0, 1)],
        "a binary operator on a unary node": [C0, (M.UNARY, M.OP["ADD"], 0, 0)],
        "node kind outside the enum": [C0, (4, 0, 0, 0)],
    }
    for what, nodes in cases.items():
        assert result_dtype(nodes, [M.INT32, M.INT32]) == GX_EINVAL, what
        assert plan(nodes, [M.INT32, M.INT32])[0] == GX_EINVAL, what
        assert compute(nodes, i32, out_dtype=M.INT32) == GX_EINVAL, what
        assert compute(nodes, i32, out_dtype=M.INT32, n=0) == GX_EINVAL, what
    from cudf_amd import _lib as L
    assert L.lib.gx_expr_result_dtype(None, 3, _i32([4, 4]), 2, None, 0) == GX_EINVAL
    assert L.lib.gx_expr_result_dtype(_node_array(good), 0, _i32([4, 4]), 2, None, 0) == GX_EINVAL
    assert L.lib.gx_expr_result_dtype(_node_array(good), 3, None, 2, None, 0) == GX_EINVAL
    # rows, pointers, begin bits
    for n in (-1, 2**31, 2**40):
        assert compute(good, i32, n=n) == GX_EINVAL, n
    assert compute(good, i32, out=None) == GX_EINVAL
    assert compute(good, [(M.INT32, None, 0), i32[1]]) == GX_EINVAL and compute(good, [i32[0], (M.INT32, None, 0)]) == GX_EINVAL
    assert compute(good, [(M.INT32, 0x10000, -1), i32[1]]) == GX_EINVAL
    assert compute([C0, L0, B("ADD", 0, 1)], i32[:1], [(M.INT32, None)]) == GX_EINVAL
    # no rows: 0, whatever the pointers, and no pointer is read
    assert compute(good, [(M.INT32, None, 0)] * 2, n=0, out=None) == 0
    assert compute([C0, L0, B("ADD", 0, 1)], [(M.INT32, None, 0)], [(M.INT32, None)], n=0, out=None) == 0
    # the plan's own arguments
    assert plan(good, [M.INT32, M.INT32], capacity=2)[0] == 0
    rc, ins, ns, ni = plan(good, [M.INT32, M.INT32], capacity=1)
    assert rc == GX_EOVERFLOW and ni == 2


def test_type_errors_are_edtype():
    two = lambda a, b: [a, b]  # noqa: E731
    for l in M.DTYPES:
        for r in M.DTYPES:
            for op in M.BINARY_OPS:
                want = M.result_dtype(op, l) if l == r else None
                got = result_dtype([C0, C1, B(op, 0, 1)], two(l, r))
                assert got == (GX_EDTYPE if want is None else want), (op, l, r)
    for t in M.DTYPES:
        for op in M.UNARY_OPS:
            want = M.result_dtype(op, t)
            assert result_dtype([C0, U(op, 0)], [t]) == (GX_EDTYPE if want is None else want), (op, t)
        for op in M.NOT_BUILT:
            assert result_dtype([C0, U(op, 0)], [t]) == GX_EDTYPE
            assert compute([C0, U(op, 0)], [(t, 0x10000, 0)], out_dtype=t) == GX_EDTYPE
    for d in (0, 12, 99, -3):
        assert result_dtype([C0], [d]) == GX_EDTYPE and result_dtype([L0], [], [d]) == GX_EDTYPE
    # a node the root does not reach is typed all the same
    assert result_dtype([C0, C1, B("ADD", 0, 1), U("IDENTITY", 0)], [M.INT32, M.INT64]) == GX_EDTYPE
    # out_dtype must be the result's: there is no cast on the final store
    add = [C0, C1, B("ADD", 0, 1)]
    i8 = [(M.INT8, 0x10000, 0), (M.INT8, 0x20000, 0)]
    assert compute(add, i8, out_dtype=M.INT8) == GX_EDTYPE and compute(add, i8, out_dtype=99) == GX_EDTYPE
    assert compute(add, i8, out_dtype=M.INT32, n=0) == 0
    # malformed beats mistyped
    assert result_dtype([C0, C1, B("ADD", 0, 2)], [M.INT32, M.INT64]) == GX_EINVAL


def test_bare_roots_and_small_plans():
    assert plan([C0], [M.INT8])[:3] == (0, [(M.LOAD, 0, M.SRC_COLUMN, 0, M.INT8, M.INT8)], 0)
    assert plan([L0], [], [M.FLOAT32])[:3] == (0, [(M.LOAD, 0, M.SRC_LITERAL, 0, M.FLOAT32, M.FLOAT32)], 0)
    # a - b: the accumulator on the left; lit - (a - b): the accumulator on the right
    rc, ins, ns, _ = plan([C0, C1, B("SUB", 0, 1), L0, B("SUB", 3, 2)], [M.INT64, M.INT64], [M.INT64])
    assert (rc, ns) == (0, 0)
    assert ins == [(M.LOAD, 0, M.SRC_COLUMN, 0, M.INT64, M.INT64), (M.APPLY, M.OP["SUB"], M.SRC_COLUMN, 1, M.INT64, M.INT64),
                   (M.APPLY_REV, M.OP["SUB"], M.SRC_LITERAL, 0, M.INT64, M.INT64)]
    # (a + b) * (c + d): one spill, and the product reads the slot on the left
    nodes = [C0, C1, B("ADD", 0, 1), (M.COLUMN, 0, 2, 0), (M.COLUMN, 0, 3, 0), B("ADD", 3, 4), B("MUL", 2, 5)]
    rc, ins, ns, _ = plan(nodes, [M.FLOAT64] * 4)
    assert (rc, ns) == (0, 1) and [i[0] for i in ins] == [M.LOAD, M.APPLY, M.SPILL, M.LOAD, M.APPLY, M.APPLY_REV]
    assert ins[-1][2:4] == (M.SRC_SLOT, 0)
    # a * a + b * b: the same column twice is no spill by itself, two products are
    nodes = [C0, B("MUL", 0, 0), C1, B("MUL", 2, 2), B("ADD", 1, 3)]
    assert plan(nodes, [M.FLOAT64] * 2)[2] == 1


# ------------------------------------------------------------------------------------------------ the plan against the model
def _random_case(rng, k):
    if k % 50 == 0:                                              # constructed: every slot index, through shared nodes
        depth = 1 + (k // 50) % 4
        nodes = _spill_tree(depth)
        t = int(rng.choice([M.INT8, M.INT64, M.FLOAT64, M.UINT32]))
        op = ["SUB", "DIV", "LESS", "TRUE_DIV"][k // 200 % 4]
        nodes = nodes[:-1] + [B(op, nodes[-1][2], nodes[-1][3])]
        return nodes, [t], []
    n_leaves = int(rng.integers(1, 9))
    n_ops = int(rng.integers(0, 32 - n_leaves + 1))
    return M.random_nodes(rng, n_ops, n_leaves, share=float(rng.choice([0.0, 0.05, 0.15])))


def test_plan_matches_a_recursive_evaluation_of_the_tree():
    rng = np.random.default_rng(20260)
    n = 67
    kinds, slots_seen, src_kinds, ops_seen, ran, too_big = set(), set(), set(), set(), 0, 0
    for k in range(2000):
        nodes, col_dtypes, lit_dtypes = _random_case(rng, k)
        want_instr, want_slots, strahler = M.expansion(nodes)
        rc, ins, ns, ni = plan(nodes, col_dtypes, lit_dtypes)
        if want_instr > 64 or want_slots > 4:
            assert rc == GX_EINVAL, (k, want_instr, want_slots)
            too_big += 1
            continue
        assert rc == 0, (k, rc, nodes)
        assert (ni, ns) == (want_instr, want_slots) and ns <= strahler, (k, ni, ns, want_instr, want_slots, strahler)
        assert result_dtype(nodes, col_dtypes, lit_dtypes) == M.node_types(nodes, col_dtypes, lit_dtypes)[-1] == ins[-1][5]
        cols = [M.random_operand(rng, t, n, null_fraction=float(rng.choice([0.0, 0.3, 1.0], p=[0.3, 0.6, 0.1]))) for t in col_dtypes]
        lits = [M.random_operand(rng, t, n, null_fraction=0.2, scalar=True) for t in lit_dtypes]
        want_v, want_ok = M.evaluate_tree(nodes, cols, lits, n)
        got_v, got_ok = M.run_plan(ins, ns, cols, lits, n)
        assert got_v.dtype == want_v.dtype, (k, got_v.dtype, want_v.dtype)
        np.testing.assert_array_equal(got_ok, want_ok, err_msg=str((k, nodes)))
        assert np.array_equal(got_v[want_ok].view(np.uint8), want_v[want_ok].view(np.uint8)) or \
            np.array_equal(got_v[want_ok], want_v[want_ok], equal_nan=True), (k, nodes)
        ran += 1
        kinds |= {i[0] for i in ins}
        slots_seen |= {i[3] for i in ins if i[0] == M.SPILL}
        src_kinds |= {i[2] for i in ins if i[0] in (M.LOAD, M.APPLY, M.APPLY_REV)}
        ops_seen |= {M.AST_OPS[i[1]] for i in ins if i[0] in (M.APPLY, M.APPLY_REV, M.APPLY_UNARY)}
    assert kinds == {M.LOAD, M.APPLY, M.APPLY_REV, M.APPLY_UNARY, M.SPILL}
    assert slots_seen == {0, 1, 2, 3} and src_kinds == {M.SRC_COLUMN, M.SRC_LITERAL, M.SRC_SLOT}
    assert ops_seen == {o for o in M.AST_OPS if o not in M.NOT_BUILT}
    assert ran >= 1500 and too_big >= 1, (ran, too_big)


# ------------------------------------------------------------------------------------------------ the C++ surface, the parser
def test_cpp_host_cases_run_without_a_device():
    r = subprocess.run([BIN, "--host"], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert ", 0 failed" in r.stdout
    assert "[ OK ] compute_column: operands of different types throw cudf::data_type_error" in r.stdout


def test_public_headers_compile_clean(tmp_path):
    inc = ["-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include"]
    c = tmp_path / "abi.c"
    c.write_text("#include <cudf_amd/gx.h>\nint main(void) { return GX_AST_CAST_TO_FLOAT64 == 49 && sizeof(gx_expr_instr) == 8 ? 0 : 1; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", *inc, str(c)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for h in ("cudf/transform.hpp", "cudf/ast/expressions.hpp"):
        cpp = tmp_path / "api.cpp"
        cpp.write_text(f"#include <{h}>\nint main() {{ return 0; }}\n")
        r = subprocess.run(["g++", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-fsyntax-only", *inc, str(cpp)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]


DT = {"a": np.dtype("int64"), "b": np.dtype("int64"), "x": np.dtype("float64"), "y": np.dtype("float64"), "f": np.dtype("bool"),
      "g": np.dtype("bool"), "u": np.dtype("uint32"), "v": np.dtype("uint8")}
NAMES = list(DT)


def _parsed(text):
    """(node list with operator names, column indices, literal (value, dtype) pairs, result dtype)"""
    from cudf_amd import ast as A
    expr, dt = A.parse_eval(text, DT)
    nodes, cols, lits = A.flatten(expr)
    kinds = {M.COLUMN: "col", M.LITERAL: "lit"}
    named = [(kinds[k], NAMES[cols[l]] if k == M.COLUMN else l) if k in kinds else
             ((M.AST_OPS[op], l) if k == M.UNARY else (M.AST_OPS[op], l, r)) for k, op, l, r in nodes]
    return named, [(l.value, l.dtype.name) for l in lits], dt.name


def test_eval_parser_accepted_grammar():
    assert _parsed("a * b + a") == ([("col", "a"), ("col", "b"), ("MUL", 0, 1), ("col", "a"), ("ADD", 2, 3)], [], "int64")
    assert _parsed("(x > y) & (a < 5)") == ([("col", "x"), ("col", "y"), ("GREATER", 0, 1), ("col", "a"), ("lit", 0), ("LESS", 3, 4),
                                              ("LOGICAL_AND", 2, 5)], [(5, "int64")], "bool")
    # a literal takes the dtype of the other side, on either side
    assert _parsed("2 - x") == ([("lit", 0), ("col", "x"), ("SUB", 0, 1)], [(2, "float64")], "float64")
    assert _parsed("x * -1.5")[1:] == ([(-1.5, "float64")], "float64")
    # operands of different dtypes are both cast
    assert _parsed("a + x") == ([("col", "a"), ("CAST_TO_FLOAT64", 0), ("col", "x"), ("CAST_TO_FLOAT64", 2), ("ADD", 1, 3)], [], "float64")
    assert _parsed("u + v")[0][1::2] == [("CAST_TO_UINT64", 0), ("CAST_TO_UINT64", 2)] and _parsed("u + v")[2] == "uint64"
    assert _parsed("a + u")[0][1::2] == [("CAST_TO_INT64", 0), ("CAST_TO_INT64", 2)] and _parsed("a + f")[2] == "int64"
    # the operators
    for text, op, dt in (("a / b", "TRUE_DIV", "float64"), ("a // b", "FLOOR_DIV", "float64"), ("a % b", "PYMOD", "int64"),
                         ("x ** y", "POW", "float64"), ("a == b", "EQUAL", "bool"), ("a != b", "NOT_EQUAL", "bool"),
                         ("a <= b", "LESS_EQUAL", "bool"), ("a >= b", "GREATER_EQUAL", "bool"), ("a & b", "BITWISE_AND", "int64"),
                         ("a | b", "BITWISE_OR", "int64"), ("f | g", "LOGICAL_OR", "bool"), ("f and g", "LOGICAL_AND", "bool"),
                         ("a or b", "LOGICAL_OR", "bool"), ("v - v", "SUB", "int32")):
        nodes, _, got = _parsed(text)
        assert nodes[-1][0] == op and got == dt, text
    assert _parsed("~f")[0][-1] == ("NOT", 0) and _parsed("not a")[0][-1] == ("NOT", 0) and _parsed("~a")[0][-1] == ("BIT_INVERT", 0)
    assert _parsed("f and g and (a > 1)")[0][-1][0] == "LOGICAL_AND" and _parsed("((a))")[0] == [("col", "a")]
    assert _parsed("7") == ([("lit", 0)], [(7, "int64")], "int64")


def test_eval_parser_rejections():
    from cudf_amd import ast as A
    for text, word in (("abs(a)", "Call"), ("a.b", "Attribute"), ("a[0]", "Subscript"), ("a ^ b", "BitXor"), ("a << 2", "LShift"),
                       ("a < b < 3", "chained"), ("a in b", "In"), ("a is b", "Is"), ("'s' + a", "'s'"), ("a if f else b", "IfExp"),
                       ("-a", "unary -"), ("[a, b]", "List"), ("a @ b", "MatMult"), ("lambda: a", "Lambda"), ("a +", "parse")):
        with pytest.raises(ValueError, match=word.replace("(", r"\(")):
            A.parse_eval(text, DT)
    with pytest.raises(KeyError):
        A.parse_eval("a + nope", DT)
    with pytest.raises(TypeError):
        A.parse_eval("a + 1.5", DT)                             # int64 cannot hold 1.5
    with pytest.raises(TypeError):
        A.parse_eval("v + 300", DT)                             # uint8 cannot hold 300
    with pytest.raises(TypeError):
        A.parse_eval("x & y", DT)
    with pytest.raises(TypeError):
        A.parse_eval("~x", DT)


def test_python_surface_rejects_bad_arguments_without_a_device():
    from cudf_amd import Column, ops
    from cudf_amd import ast as A
    i64, i32, f64 = (lambda n, dt=dt: Column(None, dt, n) for dt in (np.int64, np.int32, np.float64))
    a, b = A.ColumnReference(0), A.ColumnReference(1)
    assert ops.expression_result_dtype([i64(3), i64(3)], A.Operation("LESS", a, b)) == np.bool_
    assert ops.expression_result_dtype([i32(3)], A.Operation("TRUE_DIV", a, a)) == np.float64
    with pytest.raises(TypeError):
        ops.expression_result_dtype([i64(3), f64(3)], A.Operation("ADD", a, b))
    with pytest.raises(TypeError):
        ops.compute_column([f64(3)], A.Operation("SIN", a))
    with pytest.raises(TypeError):
        ops.compute_column([f64(3)], A.Operation("BITWISE_AND", a, a))
    with pytest.raises(IndexError):
        ops.compute_column([i64(3)], A.Operation("ADD", a, b))
    with pytest.raises(ValueError):
        ops.compute_column([i64(3), i64(4)], A.Operation("ADD", a, b))
    with pytest.raises(ValueError):
        A.Operation("PLUS", a, b)
    with pytest.raises(ValueError):
        A.Operation("ADD", a)
    with pytest.raises(ValueError):
        A.Operation("ABS", a, b)
    with pytest.raises(TypeError):
        A.Operation("ADD", a, 3)
    with pytest.raises(TypeError):
        A.Literal(300, np.int8)
    with pytest.raises(TypeError):
        A.Literal(1, np.complex64)
    with pytest.raises(ValueError):
        A.ColumnReference(-1)
    deep = a
    for _ in range(40):
        deep = A.Operation("IDENTITY", deep)
    with pytest.raises(ValueError):
        ops.expression_result_dtype([i64(3)], deep)
