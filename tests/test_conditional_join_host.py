"""CPU: the conditional joins without a device -- the symbols and their binding, every argument check of gx_conditional_join_count /
_write with fake pointers (nothing is launched), the scratch query, the tile / grid-cap queries, gx_compute_column's refusal of a
RIGHT column, the plan of a tree whichever side its columns come from, the NumPy model of the kernel's walk against the one-line
grid model, parse_eval's two-frame name resolution, ast.flatten / flatten_pair, the --host cases of the C++ binary and the header."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import conditional_join_model as CJ
from tests import expression_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EDTYPE, ETMP, EOVERFLOW = -1, -2, -3, -5
FAKE = 0x10000
NEW_SYMBOLS = ("gx_conditional_join_count", "gx_conditional_join_write", "gx_conditional_join_tile", "gx_conditional_join_grid_cap",
               "gx_conditional_join_pairs_per_run", "gx_conditional_join_set_shape")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as ge
    ge.build()
    from cudf_amd import _lib
    return _lib


def tree(L, nodes):
    return (L.ExprNode * len(nodes))(*[L.ExprNode(*nd) for nd in nodes])


def columns(L, specs):
    """specs: (dtype code, table[, data pointer[, begin bit]])"""
    out = (L.ExprColumn * max(len(specs), 1))()
    for i, s in enumerate(specs):
        out[i] = L.ExprColumn(s[2] if len(s) > 2 else FAKE, None, s[3] if len(s) > 3 else 0, s[0], s[1])
    return out


def less(L, dt=M.INT32, tables=(0, 1)):
    """l.c0 < r.c0: nodes, columns"""
    return tree(L, [(L.EXPR_COLUMN, 0, 0, 0), (L.EXPR_COLUMN, 0, 1, 0), (L.EXPR_BINARY, L.AST_OP["LESS"], 0, 1)]), \
        columns(L, [(dt, tables[0]), (dt, tables[1])])


def count(L, nodes, cols, n_cols, n_left, n_right, kind, sizes=FAKE, tmp=None, nbytes=None, lits=None, n_lits=0):
    nb = ctypes.c_size_t(0) if nbytes is None else nbytes
    rc = L.lib.gx_conditional_join_count(nodes, len(nodes), cols, n_cols, lits, n_lits, n_left, n_right, kind, sizes, tmp, ctypes.byref(nb), None)
    return rc, nb.value


def test_symbols_exported_and_bound(L):
    lib = ctypes.CDLL(os.path.join(ROOT, "cudf_amd", "libcudf_amd.so"))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in L.EXPORTED
    assert [f[0] for f in L.ExprColumn._fields_] == ["data", "valid", "begin_bit", "dtype", "table"]


def test_tile_grid_cap_and_shape_knob(L):
    tl, tr = ctypes.c_int(0), ctypes.c_int(0)
    L.lib.gx_conditional_join_tile(ctypes.byref(tl), ctypes.byref(tr))
    r = L.lib.gx_conditional_join_pairs_per_run()
    assert tl.value % 64 == 0 and tr.value % 64 == 0 and tl.value <= 1024
    assert r in (2, 4, 8) and tr.value % r == 0 and 32 % r == 0
    assert L.lib.gx_conditional_join_grid_cap() >= 256
    L.lib.gx_conditional_join_tile(None, None)                   # both pointers are optional
    for bad in ((3, 0, 0), (16, 0, 0), (4, 100, 0), (4, 0, 32), (4, 512, 0), (-1, 0, 0)):
        assert L.lib.gx_conditional_join_set_shape(*bad) == EINVAL, bad
    try:
        assert L.lib.gx_conditional_join_set_shape(8, 64, 128) == 0
        L.lib.gx_conditional_join_tile(ctypes.byref(tl), ctypes.byref(tr))
        assert tr.value == 128 and L.lib.gx_conditional_join_pairs_per_run() == 8
    finally:
        assert L.lib.gx_conditional_join_set_shape(0, 0, 0) == 0
    assert L.lib.gx_conditional_join_pairs_per_run() == r


def test_argument_checks_before_any_launch(L):
    """every refusal with fake device pointers: had anything been launched, the process would fault"""
    nodes, cols = less(L)
    nb = ctypes.c_size_t(1 << 30)
    for kind in range(5):
        assert count(L, nodes, cols, 2, 10, 10, kind)[0] == 0    # the query itself
    assert count(L, nodes, cols, 2, 10, 10, 5)[0] == EINVAL
    assert count(L, nodes, cols, 2, 10, 10, -1)[0] == EINVAL
    assert count(L, nodes, cols, 2, -1, 10, 0)[0] == EINVAL
    assert count(L, nodes, cols, 2, 10, 2**31, 0)[0] == EINVAL
    assert count(L, nodes, cols, 2, 2**31 - 1, 2**31 - 1, 0)[0] == 0
    assert count(L, nodes, cols, 17, 10, 10, 0)[0] == EINVAL
    assert count(L, nodes, None, 2, 10, 10, 0)[0] == EINVAL
    assert count(L, nodes, cols, 2, 10, 10, 0, lits=None, n_lits=1)[0] == EINVAL
    assert count(L, nodes, cols, 2, 10, 10, 0, lits=None, n_lits=17)[0] == EINVAL
    assert L.lib.gx_conditional_join_count(nodes, 3, cols, 2, None, 0, 10, 10, 0, FAKE, None, None, None) == EINVAL   # no tmp_bytes
    assert count(L, nodes, cols, 2, 10, 10, 0, sizes=None, tmp=FAKE, nbytes=nb)[0] == EINVAL                       # no sizes_dev
    assert count(L, nodes, cols, 2, 10, 10, 0, tmp=FAKE, nbytes=ctypes.c_size_t(8))[0] == ETMP
    assert count(L, nodes, columns(L, [(M.INT32, 0), (M.INT32, 2)]), 2, 10, 10, 0)[0] == EINVAL                    # table outside {0, 1}
    assert count(L, nodes, columns(L, [(M.INT32, 0), (M.INT32, -1)]), 2, 10, 10, 0)[0] == EINVAL
    assert count(L, nodes, columns(L, [(M.INT32, 0), (M.INT32, 1, FAKE, -1)]), 2, 10, 10, 0)[0] == EINVAL          # negative begin bit
    assert count(L, nodes, columns(L, [(M.INT32, 0), (M.INT32, 1, None)]), 2, 10, 10, 0)[0] == EINVAL              # NULL data with rows
    assert count(L, nodes, columns(L, [(M.INT32, 0), (M.INT32, 1, None)]), 2, 10, 0, 0)[0] == 0                    # ... an empty side is not read
    assert count(L, nodes, columns(L, [(M.INT32, 0, None), (M.INT32, 1)]), 2, 0, 10, 2)[0] == 0
    assert count(L, nodes, columns(L, [(M.INT32, 0), (M.INT64, 1)]), 2, 10, 10, 0)[0] == EDTYPE                    # operands differ
    assert count(L, nodes, columns(L, [(M.INT32, 0), (99, 1)]), 2, 10, 10, 0)[0] == EDTYPE
    add = tree(L, [(L.EXPR_COLUMN, 0, 0, 0), (L.EXPR_COLUMN, 0, 1, 0), (L.EXPR_BINARY, L.AST_OP["ADD"], 0, 1)])
    assert count(L, add, cols, 2, 10, 10, 0)[0] == EDTYPE                                                           # not BOOL8
    sin = tree(L, [(L.EXPR_COLUMN, 0, 0, 0), (L.EXPR_UNARY, L.AST_OP["SIN"], 0, 0)])
    assert count(L, sin, columns(L, [(M.FLOAT64, 1)]), 1, 10, 10, 0)[0] == EDTYPE                                   # not built
    bad_child = tree(L, [(L.EXPR_COLUMN, 0, 0, 0), (L.EXPR_BINARY, L.AST_OP["LESS"], 0, 1)])
    assert count(L, bad_child, cols, 2, 10, 10, 0)[0] == EINVAL
    out_of_range = tree(L, [(L.EXPR_COLUMN, 0, 2, 0), (L.EXPR_COLUMN, 0, 1, 0), (L.EXPR_BINARY, L.AST_OP["LESS"], 0, 1)])
    assert count(L, out_of_range, cols, 2, 10, 10, 0)[0] == EINVAL
    many = tree(L, [(L.EXPR_COLUMN, 0, 0, 0)] + [(L.EXPR_UNARY, L.AST_OP["IDENTITY"], i, 0) for i in range(32)])
    assert count(L, many, cols, 2, 10, 10, 0)[0] == EINVAL                                                          # 33 nodes

    def write(nodes, cols, n_cols, n_left, n_right, kind, total, left_total, tmp=FAKE, out_l=FAKE, out_r=FAKE):
        return L.lib.gx_conditional_join_write(nodes, len(nodes), cols, n_cols, None, 0, n_left, n_right, kind, total, left_total, tmp,
                                               out_l, out_r, None)
    assert write(nodes, cols, 2, 10, 10, 7, 5, 5) == EINVAL
    assert write(add, cols, 2, 10, 10, 0, 5, 5) == EDTYPE
    assert write(nodes, cols, 2, 10, 10, 0, -1, -1) == EINVAL
    assert write(nodes, cols, 2, 10, 10, 0, 5, 6) == EINVAL                                                         # left part above the total
    assert write(nodes, cols, 2, 10, 10, 0, 2**31, 2**31) == EOVERFLOW                                              # before anything is launched
    assert write(nodes, cols, 2, 10, 10, 2, 2**31 + 5, 7) == EOVERFLOW
    assert write(nodes, cols, 2, 10, 10, 0, 0, 0, tmp=None, out_l=None, out_r=None) == 0                            # nothing to write
    assert write(nodes, cols, 2, 10, 10, 0, 5, 5, tmp=None) == EINVAL
    assert write(nodes, cols, 2, 10, 10, 0, 5, 5, out_l=None) == EINVAL
    assert write(nodes, cols, 2, 10, 10, 1, 5, 5, out_r=None) == EINVAL


def test_scratch_query_is_monotone_in_both_row_counts(L):
    nodes, cols = less(L)
    rows = (0, 1, 63, 64, 65, 4095, 4096, 4097, 10**6, 10**8, 2**31 - 1)
    for kind in range(5):
        size = {(a, b): count(L, nodes, cols, 2, a, b, kind) for a, b in itertools.product(rows, rows)}
        assert all(rc == 0 and nbytes > 0 for rc, nbytes in size.values())
        for (a, b), (_, nbytes) in size.items():
            for a2, b2 in itertools.product(rows, rows):
                if a2 >= a and b2 >= b:
                    assert size[(a2, b2)][1] >= nbytes, (kind, a, b, a2, b2)
    # the pair joins keep 4 bytes per left row, FULL one bit per right row on top, SEMI / ANTI one bit per left row
    big = 10**8
    assert count(L, nodes, cols, 2, big, 0, 0)[1] >= 4 * big
    assert count(L, nodes, cols, 2, 0, big, 2)[1] >= big // 8 > count(L, nodes, cols, 2, 0, big, 1)[1]
    assert big // 8 <= count(L, nodes, cols, 2, big, 0, 3)[1] < 4 * big


def test_compute_column_refuses_a_right_column(L):
    nodes, cols = less(L)
    args = (nodes, 3, cols, 2, None, 0, 10, M.BOOL8, FAKE, None, None, None)
    assert L.lib.gx_compute_column(*args) == EINVAL
    nodes, cols = less(L, tables=(0, 0))
    assert L.lib.gx_compute_column(nodes, 3, cols, 2, None, 0, -1, M.BOOL8, FAKE, None, None, None) == EINVAL     # still its own checks
    assert L.lib.gx_compute_column(nodes, 3, cols, 2, None, 0, 0, M.BOOL8, None, None, None, None) == 0           # table 0, no rows: fine


def test_plan_does_not_depend_on_the_side(L):
    """gx_expr_plan sees dtypes alone: one program for a tree whichever table its columns come from"""
    from cudf_amd import ast as A
    rng = np.random.default_rng(5)
    for trial in range(20):
        nodes_m, col_dt, lit_dt = M.random_nodes(rng, int(rng.integers(1, 12)), int(rng.integers(1, 6)))
        nodes = tree(L, nodes_m)
        cd = (ctypes.c_int32 * max(len(col_dt), 1))(*col_dt)
        ld = (ctypes.c_int32 * max(len(lit_dt), 1))(*lit_dt)
        ins = (L.ExprInstr * 64)()
        n_ins, n_slots = ctypes.c_int(0), ctypes.c_int(0)
        rc = L.lib.gx_expr_plan(nodes, len(nodes_m), cd, len(col_dt), ld, len(lit_dt), ins, 64, ctypes.byref(n_ins), ctypes.byref(n_slots))
        if rc != 0:
            continue
        result = L.lib.gx_expr_result_dtype(nodes, len(nodes_m), cd, len(col_dt), ld, len(lit_dt))
        lits = (L.ExprLiteral * max(len(lit_dt), 1))(*[L.ExprLiteral(FAKE, None, d, 0) for d in lit_dt])
        for sides in ([0] * len(col_dt), [1] * len(col_dt), [i % 2 for i in range(len(col_dt))]):
            cols = columns(L, [(d, s) for d, s in zip(col_dt, sides)])
            rc2, _ = count(L, nodes, cols, len(col_dt), 5, 5, 0, lits=lits, n_lits=len(lit_dt))
            assert rc2 == (0 if result == M.BOOL8 else EDTYPE), (trial, sides, result)
    # and through the Python layer: the same tree with its references on either side flattens to the same nodes
    for tables in (("left", "left"), ("left", "right"), ("right", "left"), ("right", "right")):
        e = A.Operation("LESS", A.Operation("ADD", A.ColumnReference(0, tables[0]), A.Literal(1, np.int32)), A.ColumnReference(0, tables[1]))
        nodes_p, cols_p, _ = A.flatten_pair(e)
        assert [n[:2] for n in nodes_p] == [(L.EXPR_COLUMN, 0), (L.EXPR_LITERAL, 0), (L.EXPR_BINARY, L.AST_OP["ADD"]),
                                            (L.EXPR_COLUMN, 0), (L.EXPR_BINARY, L.AST_OP["LESS"])]
        assert cols_p == ([(tables[0], 0)] if tables[0] == tables[1] else [(tables[0], 0), (tables[1], 0)])


def test_column_reference_table_flatten_and_flatten_pair(L):
    from cudf_amd import ast as A
    assert A.ColumnReference(3).table == "left" and A.ColumnReference(3).index == 3           # the positional form is unchanged
    assert A.ColumnReference(2, "right").table == "right" and A.ColumnReference(2, table="right").index == 2
    with pytest.raises(ValueError):
        A.ColumnReference(0, "output")
    with pytest.raises(ValueError):
        A.ColumnReference(-1, "right")
    one = A.Operation("ADD", A.ColumnReference(4), A.ColumnReference(1))
    nodes, cols, lits = A.flatten(one)
    assert cols == [4, 1] and lits == [] and len(nodes) == 3                                   # flatten's return value is unchanged
    assert A.flatten_pair(one)[1] == [("left", 4), ("left", 1)]
    two = A.Operation("LESS", A.ColumnReference(0), A.ColumnReference(0, "right"))
    assert A.flatten_pair(two)[1] == [("left", 0), ("right", 0)]                               # same index, two tables: two columns
    with pytest.raises(ValueError, match="right table"):
        A.flatten(two)
    with pytest.raises(TypeError):
        A.flatten_pair("l.a < r.b")


def test_parse_eval_resolves_names_over_two_frames(L):
    from cudf_amd import ast as A
    left = {"a": np.dtype(np.int32), "v": np.dtype(np.float64), "lo": np.dtype(np.int64)}
    right = {"b": np.dtype(np.int32), "v": np.dtype(np.float64), "t": np.dtype(np.int8)}
    e, dt = A.parse_eval("a < b", left, right)
    assert dt == np.bool_ and A.flatten_pair(e)[1] == [("left", 0), ("right", 0)]
    e, dt = A.parse_eval("left.v > right.v and lo <= t", left, right)
    assert dt == np.bool_ and A.flatten_pair(e)[1] == [("left", 1), ("right", 1), ("left", 2), ("right", 2)]
    nodes = A.flatten_pair(e)[0]
    assert [L.AST_OPS[n[1]] for n in nodes if n[0] == L.EXPR_UNARY] == ["CAST_TO_INT64"] * 2  # int64 lo against int8 t: unify casts both sides
    e, dt = A.parse_eval("left.a + right.b", left, right)
    assert dt == np.int32
    with pytest.raises(ValueError, match="both frames"):
        A.parse_eval("v > 1.0", left, right)
    with pytest.raises(KeyError):
        A.parse_eval("a < nothing", left, right)
    with pytest.raises(KeyError):
        A.parse_eval("left.b < 1", left, right)
    with pytest.raises(KeyError):
        A.parse_eval("right.a < 1", left, right)
    # one frame: unchanged, and `left.` is not a name there
    e, dt = A.parse_eval("a < 3", left)
    assert A.flatten(e)[1] == [0]
    with pytest.raises(ValueError):
        A.parse_eval("left.a < 3", left)


@pytest.mark.parametrize("kind", CJ.KINDS)
def test_walk_model_equals_the_grid_model_exhaustively(kind):
    """the tile / segment / chunk / R walk with a capped grid against the one-line model, for every (n_left, n_right) up to
    (2 TL' + 1, 2 TR' + 1) on a scaled-down shape; three densities, so that rows with no, one and many matches occur"""
    TL, TR, R, cap = 4, 6, 2, 2
    rng = np.random.default_rng(7)
    full = [rng.random((2 * TL + 1, 2 * TR + 1)) < p for p in (0.08, 0.5, 1.0)]
    for nl in range(2 * TL + 2):
        for nr in range(2 * TR + 2):
            for m in full:
                m = m[:nl, :nr]
                want = CJ.join_of(m, kind)
                for per in (1, 2):                              # one chunk per segment, and two
                    got, total = CJ.walk_join(m, kind, TL, TR, R, cap, per)
                    if isinstance(want, tuple):
                        assert total == len(want[0])
                        assert (got[0] == want[0]).all() and (got[1] == want[1]).all(), (nl, nr, per)
                    else:
                        assert total == len(want) and (got == want).all(), (nl, nr, per)


def test_grid_model_on_hand_written_cases():
    """the oracle of the GPU tests, held to pairs written out by hand: nulls, NULL_EQUAL, IS_NULL, a literal"""
    a = (np.array([0, 1, 2, 1], dtype=np.int32), np.array([1, 0, 1, 1], dtype=bool))
    b = (np.array([1, 2, 7], dtype=np.int32), np.array([1, 1, 0], dtype=bool))
    col = [("left", 0), ("right", 0)]
    eq = [(M.COLUMN, 0, 0, 0), (M.COLUMN, 0, 1, 0), (M.BINARY, M.OP["EQUAL"], 0, 1)]
    m = CJ.grid_matches(eq, col, [a], [b], [])
    assert [tuple(p) for p in np.argwhere(m)] == [(2, 1), (3, 0)]
    neq = eq[:2] + [(M.BINARY, M.OP["NULL_EQUAL"], 0, 1)]
    assert [tuple(p) for p in np.argwhere(CJ.grid_matches(neq, col, [a], [b], []))] == [(1, 2), (2, 1), (3, 0)]
    isn = [(M.COLUMN, 0, 0, 0), (M.UNARY, M.OP["IS_NULL"], 0, 0)]
    assert [tuple(p) for p in np.argwhere(CJ.grid_matches(isn, [("right", 0)], [a], [b], []))] == [(i, 2) for i in range(4)]
    l, r = CJ.join_of(m, "full")
    assert list(l) == [0, 1, 2, 3, CJ.NO_MATCH] and list(r) == [CJ.NO_MATCH, CJ.NO_MATCH, 1, 0, 2]
    assert list(CJ.join_of(m, "leftsemi")) == [2, 3] and list(CJ.join_of(m, "leftanti")) == [0, 1]
    lit = [(M.LITERAL, 0, 0, 0)]
    assert CJ.grid_matches(lit, [], [a], [b], [(np.array([True]), np.array([True]))]).all()
    assert not CJ.grid_matches(lit, [], [a], [b], [(np.array([True]), np.array([False]))]).any()


def test_cpp_host_cases(L):
    binary = os.path.join(ROOT, "tests", "cpp", "cudf_conditional_join_tests")
    assert os.path.exists(binary), "build() makes it"
    res = subprocess.run([binary, "--host"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and ", 0 failed" in res.stdout, res.stdout[-3000:] + res.stderr[-2000:]
    assert res.stdout.count("[ OK ]") >= 5


def test_new_header_compiles_clean(tmp_path):
    cpp = tmp_path / "one.cpp"
    cpp.write_text("#include <cudf/join/conditional_join.hpp>\nint main() { return 0; }\n")
    inc = [f"-I{os.path.join(ROOT, 'include')}", "-I/opt/rocm/include"]
    r = subprocess.run(["g++", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-fsyntax-only", *inc, str(cpp)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
