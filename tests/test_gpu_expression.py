"""GPU: cudf::compute_column -- ops.compute_column, DataFrame.eval / query and gx_compute_column under them
(cudf_amd/csrc/gx_expression.hip), plus the C++ surface (tests/cpp/cudf_transform_tests).
The oracle is the UNFUSED CHAIN: ops.binary_operation(..., out_dtype = the rule's dtype), ops.unary_operation, ops.cast and
ops.is_null node by node (tests/test_gpu_elementwise.py holds those to NumPy); FLOOR_DIV is the chain TRUE_DIV then FLOOR, ABS and
BIT_INVERT on narrow types are cast to the compute class first.  A handful of cases are checked against NumPy directly as well, so
that the oracle and the feature cannot share an error.  Per case: valid rows bit for bit (two NaNs are equal), the validity words
in full with a guard word behind them, the null count, and the bytes behind the last row.  The fused call goes through the C ABI
(so that begin bits and unaligned views can be given) and through ops.compute_column.  Row counts come from
T = gx_expression_tile_rows()."""
import ctypes
import itertools
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import expression_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ["int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float32", "float64", "bool"]
INTS, FLOATS = DTYPES[:8], ["float32", "float64"]
BEGIN_BITS = (0, 1, 31, 33)
BIG = 2**22 + 4097
GUARD_WORD, GUARD_BYTE = 0x5EEDFACE, 0xA5


@pytest.fixture(scope="module")
def gx():
    import cudf_amd
    from cudf_amd import Column, ops
    from cudf_amd import ast as A
    return cudf_amd, Column, ops, A


@pytest.fixture(scope="module")
def T(gx):
    return int(gx[0]._lib.lib.gx_expression_tile_rows())


@pytest.fixture(scope="module")
def ROWS(T):
    return (0, 1, 31, 32, 33, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17)


def code(dt):
    return M.GX[np.dtype(dt)]


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_same(got, want, what="", valid=None):
    """bit for bit on the valid rows; NaN == NaN"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    eq = bits_of(got) == bits_of(want)
    if got.dtype.kind == "f":
        eq |= np.isnan(got) & np.isnan(want)
    if valid is not None:
        eq = eq | ~valid
    if not eq.all():
        i = int(np.flatnonzero(~eq)[0])
        raise AssertionError(f"{what}: {int((~eq).sum())} rows differ, first at {i}: got {got[i]!r}, want {want[i]!r}")


def values(rng, dt, n, small=False, nonneg=False):
    """n values of dt: over the whole width with the extremes among them, or small (|v| <= 50, halves for floats)"""
    dt = np.dtype(dt)
    if dt == np.bool_:
        return rng.integers(0, 2, n).astype(np.bool_)
    if small:
        lo = 0 if dt.kind == "u" or nonneg else -50
        v = rng.integers(lo * 2, 101, n) / 2
        return v.astype(dt) if dt.kind == "f" else np.trunc(v).astype(dt)
    if dt.kind == "f":
        v = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(dt)
        if n >= 8:
            v[rng.permutation(n)[:5]] = [np.nan, np.inf, -np.inf, -0.0, 0.0]
        return v
    info = np.iinfo(dt)
    v = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    edge = np.array([info.min, info.max, 0, 1, info.max - 1, info.min + 1], dtype=dt)
    k = min(n, len(edge))
    v[rng.permutation(n)[:k]] = edge[:k]
    return v


def nonzero(v):
    v = v.copy()
    v[v == 0] = 1
    if v.dtype.kind == "i":
        v[v == -1] = 2                       # never the INT_MIN / -1 pair
    return v


# ------------------------------------------------------------------------------------------------ the fused call through the C ABI
def fused_abi(gx, expr, cols, n, begin_bits=None, offsets=None, out_offset=0, with_valid=None):
    """gx_compute_column on host arrays.  cols: [(values, validity or None)] by table index; begin_bits / offsets (elements) place
    each column's bitmap and data inside larger device buffers; out_offset (elements) does the same for the output.  Checks the
    guard word behind the validity words and the bytes behind the last row.  Returns (values, validity or None, null count)."""
    import torch
    cudf_amd, Column, ops, A = gx
    L = cudf_amd._lib
    nodes, used, literals = A.flatten(expr)
    node_arr = (L.ExprNode * len(nodes))(*[L.ExprNode(*nd) for nd in nodes])
    begin_bits = begin_bits or [0] * len(cols)
    offsets = offsets or [0] * len(cols)
    keep, col_structs = [], []
    rng = np.random.default_rng(1234)
    for i in used:
        v, ok = cols[i]
        dt = v.dtype
        host = np.zeros(offsets[i] + n + 3, dtype=dt)
        host[offsets[i]:offsets[i] + n] = v
        data = torch.from_numpy(host.view(np.uint8).copy()).cuda()
        mask_ptr = None
        if ok is not None:
            bits = rng.integers(0, 2, begin_bits[i] + n + 40).astype(np.uint8)      # noise around the column's bits
            bits[begin_bits[i]:begin_bits[i] + n] = ok
            words = np.packbits(np.concatenate([bits, np.zeros((-len(bits)) % 32, np.uint8)]), bitorder="little").view(np.int32)
            mask = torch.from_numpy(words.copy()).cuda()
            keep.append(mask)
            mask_ptr = mask.data_ptr()
        keep.append(data)
        col_structs.append(L.ExprColumn(data.data_ptr() + offsets[i] * dt.itemsize, mask_ptr, begin_bits[i], code(dt), 0))
    lit_structs = []
    for l in literals:
        val, vb = ops._device_scalar(l.value, l.dtype)
        keep.append((val, vb))
        lit_structs.append(L.ExprLiteral(val.data_ptr(), vb.data_ptr(), code(l.dtype), 0))
    col_arr = (L.ExprColumn * max(len(col_structs), 1))(*col_structs)
    lit_arr = (L.ExprLiteral * max(len(lit_structs), 1))(*lit_structs)
    out_dt = ops.expression_result_dtype([Column(None, v.dtype, n) for v, _ in cols], expr)
    if with_valid is None:
        with_valid = any(cols[i][1] is not None for i in used) or any(l.value is None for l in literals)
    nbytes = (out_offset + n) * out_dt.itemsize
    out = torch.full((nbytes + 64,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
    nwords = (n + 31) // 32
    valid = torch.full((nwords + 1,), GUARD_WORD, dtype=torch.int32, device="cuda") if with_valid else None
    nulls = torch.full((1,), -7, dtype=torch.int64, device="cuda") if with_valid else None
    rc = L.lib.gx_compute_column(node_arr, len(nodes), col_arr, len(col_structs), lit_arr, len(lit_structs), n, code(out_dt),
                                 ctypes.c_void_p(out.data_ptr() + out_offset * out_dt.itemsize),
                                 ctypes.c_void_p(valid.data_ptr()) if with_valid else None,
                                 ctypes.c_void_p(nulls.data_ptr()) if with_valid else None,
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    host = out.cpu().numpy()
    assert (host[:out_offset * out_dt.itemsize] == GUARD_BYTE).all() and (host[nbytes:] == GUARD_BYTE).all(), "bytes around the rows"
    got = host[out_offset * out_dt.itemsize:nbytes].copy().view(out_dt)
    if not with_valid:
        return got, None, 0
    words = valid.cpu().numpy().view(np.uint32)
    assert words[nwords] == GUARD_WORD, "the word behind the validity words"
    ok = np.unpackbits(words[:nwords].view(np.uint8), bitorder="little").astype(bool)
    assert not ok[n:].any(), "bits behind the last row"
    null_count = int(nulls.item()) if n else 0
    return got, ok[:n], null_count


# ------------------------------------------------------------------------------------------------ the oracle: the unfused chain
BINOP_NAME = {"NULL_EQUAL": "NULL_EQUALS"}


def chain(gx, expr, cols, n):
    """node by node with the element-wise entry points; a literal is a column of n equal rows.  Returns (values, validity)."""
    _, Column, ops, A = gx
    table = [Column.from_numpy(v, ok) for v, ok in cols]
    memo = {}

    def ev(e):
        if id(e) in memo:
            return memo[id(e)]
        if isinstance(e, A.ColumnReference):
            r = table[e.index]
        elif isinstance(e, A.Literal):
            v = np.full(n, 0 if e.value is None else e.value, dtype=e.dtype)
            r = Column.from_numpy(v, None if e.value is not None else np.zeros(n, bool))
        elif e.rhs is None:
            c = ev(e.lhs)
            name = e.name
            if name == "IDENTITY":
                r = c
            elif name == "IS_NULL":
                r = ops.is_null(c)
            elif name in ("ABS", "BIT_INVERT"):
                cc = np.dtype(M.NP[M.cls(code(c.dtype))])
                r = ops.unary_operation(c if c.dtype == cc else ops.cast(c, cc), name)
            elif name.startswith("CAST_TO_"):
                r = ops.cast(c, M.NP[M.result_dtype(name, code(c.dtype))])
            else:
                r = ops.unary_operation(c, name)
        else:
            l, rr = ev(e.lhs), ev(e.rhs)
            out = M.NP[M.result_dtype(e.name, code(l.dtype))]
            if e.name == "FLOOR_DIV":
                r = ops.unary_operation(ops.binary_operation(l, rr, "TRUE_DIV", np.float64), "FLOOR")
            else:
                r = ops.binary_operation(l, rr, BINOP_NAME.get(e.name, e.name), out)
        memo[id(e)] = r
        return r

    r = ev(expr)
    ok = r.valid_numpy() if r.has_nulls() else np.ones(n, bool)
    return r.to_numpy(), ok


def check(gx, expr, cols, n, what="", **place):
    """the fused call (C ABI, and ops.compute_column when nothing is placed) against the chain"""
    _, Column, ops, A = gx
    want, want_ok = chain(gx, expr, cols, n)
    got, got_ok, nulls = fused_abi(gx, expr, cols, n, **place)
    if got_ok is None:
        got_ok = np.ones(n, bool)
        assert want_ok.all(), what
    assert np.array_equal(got_ok, want_ok), f"{what}: validity differs at {np.flatnonzero(got_ok != want_ok)[:5]}"
    assert nulls == int((~want_ok).sum()), what
    assert_same(got, want, what, want_ok)
    if not place:
        col = ops.compute_column([Column.from_numpy(v, ok) for v, ok in cols], expr)
        assert col.size == n and col.dtype == want.dtype and col.null_count == nulls and (col.mask is not None) == (nulls > 0), what
        if nulls:
            assert np.array_equal(col.valid_numpy(), want_ok), what
        assert_same(col.to_numpy(), want, what + " (ops.compute_column)", want_ok)
    return got, got_ok


def masks(rng, n, *fractions):
    return [None if f is None else rng.random(n) < f for f in fractions]


# ------------------------------------------------------------------------------------------------ row counts
def test_every_row_count_against_the_chain_and_numpy(gx, ROWS):
    """a * b + c on float64 with two bitmaps, and (a > b) & (c < 5) into BOOL8, at every row count of the set"""
    _, Column, ops, A = gx
    a, b, c = (A.ColumnReference(i) for i in range(3))
    fma = A.Operation("ADD", A.Operation("MUL", a, b), c)
    pred = A.Operation("LOGICAL_AND", A.Operation("GREATER", a, b), A.Operation("LESS", c, A.Literal(5, np.float64)))
    rng = np.random.default_rng(1)
    for n in ROWS:
        x, y, z = (values(rng, "float64", n, small=True) for _ in range(3))
        ka, kb, kc = masks(rng, n, 0.8, None, 0.5)
        got, ok = check(gx, fma, [(x, ka), (y, kb), (z, kc)], n, f"a*b+c n={n}")
        assert_same(got, x * y + z, f"a*b+c vs NumPy n={n}", ka & kc)
        assert np.array_equal(ok, ka & kc)
        got, ok = check(gx, pred, [(x, ka), (y, kb), (z, kc)], n, f"predicate n={n}")
        assert_same(got, (x > y) & (z < 5), f"predicate vs NumPy n={n}", ka & kc)
        got, ok = check(gx, pred, [(x, None), (y, None), (z, None)], n, f"predicate without masks n={n}")
        assert ok.all()


def test_second_trip_of_the_grid_and_a_large_column(gx, T):
    """grid cap x T + 1 rows on int8 (the grid-stride loop takes a second trip; the fewest bytes per tile), 2^22 + 4097 on int64"""
    cudf_amd, Column, ops, A = gx
    cap = int(cudf_amd._lib.lib.gx_expression_grid_cap())
    a, b = A.ColumnReference(0), A.ColumnReference(1)
    rng = np.random.default_rng(2)
    for dt, n in (("int8", cap * T + 1), ("int64", BIG)):
        x, y = values(rng, dt, n), values(rng, dt, n)
        ka, kb = masks(rng, n, 0.8, 0.8)
        got, ok = check(gx, A.Operation("ADD", a, b), [(x, ka), (y, kb)], n, f"{dt} n={n}")
        C = np.dtype(M.NP[M.cls(code(dt))])
        with np.errstate(over="ignore"):
            assert_same(got, x.astype(C) + y.astype(C), f"{dt} n={n} vs NumPy", ka & kb)


# ------------------------------------------------------------------------------------------------ expression shapes
def balanced(A, op, leaves):
    while len(leaves) > 1:
        leaves = [A.Operation(op, leaves[i], leaves[i + 1]) for i in range(0, len(leaves), 2)]
    return leaves[0]


def test_expression_shapes(gx, T):
    cudf_amd, Column, ops, A = gx
    rng = np.random.default_rng(3)
    n = T + 77
    r = [A.ColumnReference(i) for i in range(16)]
    f = [(nonzero(values(rng, "float64", n, small=True)), m) for m in masks(rng, n, 0.9, None, 0.7, None) + [None] * 12]
    i64 = [(nonzero(values(rng, "int64", n, small=True)), m) for m in masks(rng, n, 0.9, None, 0.7, None)]
    one = A.Literal(1.5, np.float64)
    shapes = {
        "left-deep chain": balanced(A, "ADD", r[:2]),
        "right-deep SUB / DIV": A.Operation("SUB", r[0], A.Operation("DIV", r[1], A.Operation("SUB", one, A.Operation("DIV", r[2], r[3])))),
        "the same column under both operands": A.Operation("ADD", A.Operation("MUL", r[0], r[0]), A.Operation("MUL", r[1], r[1])),
        "(a + b) * (c + d)": A.Operation("MUL", A.Operation("ADD", r[0], r[1]), A.Operation("ADD", r[2], r[3])),
        # two non-leaf children: the left side is spilled and read back on the left of the division ...
        "(a - b) / (|c| + |d|)": A.Operation("DIV", A.Operation("SUB", r[0], r[1]), A.Operation("ADD", A.Operation("ABS", r[2]), A.Operation("ABS", r[3]))),
        # ... and the heavier right side runs first: the slot is the divisor
        "(a - b) / (|c| * |c| + |d|)": A.Operation("DIV", A.Operation("SUB", r[0], r[1]),
                                                   A.Operation("ADD", A.Operation("MUL", A.Operation("ABS", r[2]), A.Operation("ABS", r[2])),
                                                               A.Operation("ABS", r[3]))),
        "balanced tree of 16 leaves": balanced(A, "SUB", r[:16]),
        "bare column": r[2],
        "bare literal": one,
        "an invalid literal root": A.Literal(None, np.int16),
    }
    left = r[0]
    for k in range(1, 4):
        left = A.Operation(("SUB", "MUL", "ADD")[k - 1], left, r[k])
    shapes["left-deep chain"] = left
    s = A.Operation("SUB", r[0], r[1])
    shapes["one node under two parents"] = A.Operation("ADD", A.Operation("MUL", s, s), A.Operation("DIV", s, r[2]))
    for what, expr in shapes.items():
        check(gx, expr, f, n, what)
    for what in ("(a - b) / (|c| + |d|)", "(a - b) / (|c| * |c| + |d|)"):
        check(gx, shapes[what], i64, n, "int64 " + what)
    # every spill slot of gx_expr_limits: each level joins two copies of the level below
    slots = ctypes.c_int(0)
    cudf_amd._lib.lib.gx_expr_limits(None, None, None, ctypes.byref(slots))
    p, q = A.Operation("ABS", r[0]), A.Operation("ABS", r[1])
    for _ in range(slots.value - 1):
        p, q = A.Operation("ADD", p, q), A.Operation("SUB", q, p)
    lvl = A.Operation("SUB", p, q)
    nodes = A.flatten(lvl)[0]
    ins = (cudf_amd._lib.ExprInstr * 64)()
    ni, ns = ctypes.c_int(0), ctypes.c_int(0)
    node_arr = (cudf_amd._lib.ExprNode * len(nodes))(*[cudf_amd._lib.ExprNode(*nd) for nd in nodes])
    cd = (ctypes.c_int32 * 2)(code("float64"), code("float64"))
    assert cudf_amd._lib.lib.gx_expr_plan(node_arr, len(nodes), cd, 2, cd, 0, ins, 64, ctypes.byref(ni), ctypes.byref(ns)) == 0
    assert ns.value == slots.value, (ns.value, slots.value)
    check(gx, lvl, f, n, "every spill slot")
    check(gx, lvl, [(v[:33], None if m is None else m[:33]) for v, m in f], 33, "every spill slot, 33 rows")


def test_one_slot_more_than_the_limit_is_an_error_and_writes_nothing(gx):
    import torch
    cudf_amd, Column, ops, A = gx
    L = cudf_amd._lib
    slots = ctypes.c_int(0)
    L.lib.gx_expr_limits(None, None, None, ctypes.byref(slots))
    lvl = A.Operation("ABS", A.ColumnReference(0))
    for _ in range(slots.value + 1):
        lvl = A.Operation("ADD", lvl, lvl)
    col = Column.from_numpy(np.arange(100, dtype=np.int64))
    with pytest.raises(ValueError):
        ops.compute_column([col], lvl)
    nodes = A.flatten(lvl)[0]
    node_arr = (L.ExprNode * len(nodes))(*[L.ExprNode(*nd) for nd in nodes])
    out = torch.full((800,), GUARD_BYTE, dtype=torch.uint8, device="cuda")
    ca = (L.ExprColumn * 1)(L.ExprColumn(col.data.data_ptr(), None, 0, code("int64"), 0))
    rc = L.lib.gx_compute_column(node_arr, len(nodes), ca, 1, (L.ExprLiteral * 1)(), 0, 100, code("int64"), ctypes.c_void_p(out.data_ptr()),
                                 None, None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == -1 and (out.cpu().numpy() == GUARD_BYTE).all()


# ------------------------------------------------------------------------------------------------ every operator, every dtype
@pytest.mark.parametrize("dt", DTYPES)
def test_every_built_operator_on_this_dtype(gx, T, dt):
    """every binary and unary operator the dtype takes, on two columns with bitmaps; divisors are nonzero and never -1, POW and the
    casts of floats see small values (out of range is unspecified)"""
    _, Column, ops, A = gx
    rng = np.random.default_rng(40 + DTYPES.index(dt))
    n = T + 33
    t = code(dt)
    a, b, d, s, p = (A.ColumnReference(i) for i in range(5))
    x, y = values(rng, dt, n), values(rng, dt, n)
    small, pos = values(rng, dt, n, small=True), values(rng, dt, n, small=True, nonneg=True)
    ka, kb = masks(rng, n, 0.8, 0.6)
    table = [(x, ka), (y, kb), (nonzero(y), kb), (small, ka), (pos, kb)]
    ran = []
    for op in M.BINARY_OPS:
        if M.result_dtype(op, t) is None:
            with pytest.raises(TypeError):
                ops.expression_result_dtype([Column(None, dt, 1)] * 2, A.Operation(op, a, b))
            continue
        lhs, rhs = (s, p) if op == "POW" else (a, d if op in ("DIV", "MOD", "PYMOD", "TRUE_DIV", "FLOOR_DIV") else b)
        check(gx, A.Operation(op, lhs, rhs), table, n, f"{op} {dt}")
        ran.append(op)
    for op in M.UNARY_OPS:
        if M.result_dtype(op, t) is None:
            with pytest.raises(TypeError):
                ops.expression_result_dtype([Column(None, dt, 1)], A.Operation(op, a))
            continue
        src = a
        if np.dtype(dt).kind == "f" and op.startswith("CAST_TO_"):
            src = p if op == "CAST_TO_UINT64" else s
        check(gx, A.Operation(op, src), table, n, f"{op} {dt}")
        ran.append(op)
    assert len(ran) >= 27


def test_pinned_values_against_numpy(gx):
    """~a on uint8 is the int of C++, abs(int8 -128) is 128, FLOOR_DIV on negative integers is floor(double / double)"""
    _, Column, ops, A = gx
    a, b = A.ColumnReference(0), A.ColumnReference(1)
    u8 = np.array([0, 1, 255, 128, 7], np.uint8)
    got = ops.compute_column([Column.from_numpy(u8)], A.Operation("BIT_INVERT", a))
    assert got.dtype == np.int32 and got.to_numpy().tolist() == [-1, -2, -256, -129, -8]
    i8 = np.array([-128, -1, 0, 127, -127], np.int8)
    got = ops.compute_column([Column.from_numpy(i8)], A.Operation("ABS", a))
    assert got.dtype == np.int32 and got.to_numpy().tolist() == [128, 1, 0, 127, 127]
    x = np.array([7, -7, 7, -7, 1, -1, 0, -9], np.int64)
    y = np.array([2, 2, -2, -2, 3, 3, 5, 4], np.int64)
    got = ops.compute_column([Column.from_numpy(x), Column.from_numpy(y)], A.Operation("FLOOR_DIV", a, b))
    assert got.dtype == np.float64 and got.to_numpy().tolist() == [3.0, -4.0, -4.0, 3.0, 0.0, -1.0, 0.0, -3.0]
    assert got.to_numpy().tolist() == np.floor(x / y).tolist()
    got = ops.compute_column([Column.from_numpy(x), Column.from_numpy(y)], A.Operation("DIV", a, b))
    assert got.dtype == np.int64 and got.to_numpy().tolist() == [3, -3, -3, 3, 0, 0, 0, -2]          # '/' of C++ truncates
    got = ops.compute_column([Column.from_numpy(x), Column.from_numpy(y)], A.Operation("PYMOD", a, b))
    assert got.to_numpy().tolist() == (x % y).tolist()
    got = ops.compute_column([Column.from_numpy(x), Column.from_numpy(y)], A.Operation("TRUE_DIV", a, b))
    assert got.dtype == np.float64 and got.to_numpy().tolist() == (x / y).tolist()


# ------------------------------------------------------------------------------------------------ widths, alignment
def test_mixed_widths_in_one_expression(gx, T):
    """int8 columns cast to INT64 beside a float64 column (narrow loads at 2 rows per access), BOOL8 out of 8-byte inputs (a narrow
    store at 2 rows per access), and 8-byte intermediates between int8 inputs and a BOOL8 output (16 rows per access)"""
    _, Column, ops, A = gx
    rng = np.random.default_rng(5)
    n = 2 * T + 19
    a8, b8, x = values(rng, "int8", n), values(rng, "int8", n), values(rng, "float64", n, small=True)
    ka, kb, kx = masks(rng, n, 0.7, None, 0.9)
    a, b, c = (A.ColumnReference(i) for i in range(3))
    table = [(a8, ka), (b8, kb), (x, kx)]
    s = A.Operation("MUL", A.Operation("CAST_TO_INT64", a), A.Operation("CAST_TO_INT64", b))
    got, ok = check(gx, A.Operation("ADD", A.Operation("CAST_TO_FLOAT64", s), c), table, n, "int8 -> INT64 beside float64")
    assert_same(got, (a8.astype(np.int64) * b8.astype(np.int64)).astype(np.float64) + x, "vs NumPy", ok)
    check(gx, A.Operation("LESS", c, A.Operation("CAST_TO_FLOAT64", s)), table, n, "BOOL8 out of 8-byte inputs")
    big = A.Literal(2**40, np.int64)
    got, ok = check(gx, A.Operation("LESS", A.Operation("MUL", s, big), big), table[:2], n, "int8 -> INT64 -> BOOL8")
    assert_same(got, a8.astype(np.int64) * b8.astype(np.int64) * 2**40 < 2**40, "vs NumPy", ok)
    check(gx, A.Operation("ADD", a, b), table[:2], n, "int8 + int8 -> INT32")


@pytest.mark.parametrize("dt", ["int8", "int16", "float32", "float64"])
def test_unaligned_views(gx, T, dt):
    """data that starts 1 or 3 elements into an aligned buffer, and an output that does: element accesses, the same values"""
    _, Column, ops, A = gx
    rng = np.random.default_rng(6)
    n = T + 45
    x, y = values(rng, dt, n, small=True), values(rng, dt, n, small=True)
    ka, kb = masks(rng, n, 0.8, None)
    a, b = A.ColumnReference(0), A.ColumnReference(1)
    expr = A.Operation("SUB", A.Operation("MUL", a, b), A.Operation("MUL", b, b))
    for offs, out_off in (([1, 0], 0), ([3, 1], 0), ([0, 0], 1), ([1, 3], 3)):
        check(gx, expr, [(x, ka), (y, kb)], n, f"{dt} offsets {offs} out {out_off}", offsets=offs, out_offset=out_off, begin_bits=[offs[0], 0])


# ------------------------------------------------------------------------------------------------ type errors
# the result of every operator by dtype, written out: "class" = C(T), "same" = T; a second word restricts the dtypes that are taken
RESULT = {"ADD": "class", "SUB": "class", "MUL": "class", "DIV": "class", "MOD": "class", "PYMOD": "class", "TRUE_DIV": "float64",
          "FLOOR_DIV": "float64", "POW": "pow", "BITWISE_AND": "class integers", "BITWISE_OR": "class integers", "BITWISE_XOR": "class integers",
          "EQUAL": "bool", "NOT_EQUAL": "bool", "LESS": "bool", "GREATER": "bool", "LESS_EQUAL": "bool", "GREATER_EQUAL": "bool",
          "LOGICAL_AND": "bool", "LOGICAL_OR": "bool", "NULL_EQUAL": "bool", "NULL_LOGICAL_AND": "bool", "NULL_LOGICAL_OR": "bool",
          "IDENTITY": "same", "IS_NULL": "bool", "NOT": "bool", "ABS": "class numbers", "BIT_INVERT": "class integers-not-bool",
          "SQRT": "same floats", "CEIL": "same floats", "FLOOR": "same floats", "RINT": "same floats", "CAST_TO_INT64": "int64",
          "CAST_TO_UINT64": "uint64", "CAST_TO_FLOAT64": "float64"}
CLASS = {"int8": "int32", "int16": "int32", "uint8": "int32", "uint16": "int32", "bool": "int32"}


def table_result(op, dt):
    rule = RESULT.get(op)
    if rule is None:
        return None
    kind, _, only = rule.partition(" ")
    taken = {"": True, "integers": dt in INTS or dt == "bool", "integers-not-bool": dt in INTS, "numbers": dt != "bool",
             "floats": dt in FLOATS}[only]
    if not taken:
        return None
    if kind == "pow":
        return "float32" if dt == "float32" else "float64"
    return {"class": CLASS.get(dt, dt), "same": dt}.get(kind, kind)


def test_result_dtype_table_and_type_errors(gx):
    _, Column, ops, A = gx
    a, b = A.ColumnReference(0), A.ColumnReference(1)
    col = lambda dt: Column(None, dt, 3)  # noqa: E731
    for op in M.AST_OPS:
        unary = op in M.UNARY_OPS
        for dt in DTYPES:
            expr = A.Operation(op, a) if unary else A.Operation(op, a, b)
            want = table_result(op, dt)
            if want is None:
                with pytest.raises(TypeError):
                    ops.expression_result_dtype([col(dt), col(dt)], expr)
                with pytest.raises(TypeError):
                    ops.compute_column([col(dt), col(dt)], expr)
            else:
                assert ops.expression_result_dtype([col(dt), col(dt)], expr) == np.dtype(want), (op, dt)
    for l, r in itertools.permutations(DTYPES, 2):               # every mismatched operand pair
        for op in ("ADD", "LESS", "NULL_EQUAL", "LOGICAL_AND"):
            with pytest.raises(TypeError):
                ops.compute_column([col(l), col(r)], A.Operation(op, a, b))
    assert set(M.NOT_BUILT) == {op for op in M.AST_OPS if op not in RESULT}


# ------------------------------------------------------------------------------------------------ validity
def test_begin_bits_independently_per_column(gx, T):
    _, Column, ops, A = gx
    rng = np.random.default_rng(7)
    n = T + 65
    a, b, c = (A.ColumnReference(i) for i in range(3))
    expr = A.Operation("ADD", A.Operation("MUL", a, b), A.Operation("MUL", c, c))
    for dt in ("int32", "float64", "int8"):
        table = [(values(rng, dt, n, small=True), m) for m in masks(rng, n, 0.5, 0.5, 0.9)]
        for bits in itertools.product(BEGIN_BITS, BEGIN_BITS, (0, 33)):
            check(gx, expr, table, n, f"{dt} begin bits {bits}", begin_bits=list(bits))


def test_validity_mixes_and_the_null_aware_operators(gx, T):
    _, Column, ops, A = gx
    rng = np.random.default_rng(8)
    n = T + 65
    a, b, c, d = (A.ColumnReference(i) for i in range(4))
    x, y, z, w = (values(rng, "int32", n, small=True) for _ in range(4))
    flag = values(rng, "bool", n)
    add = A.Operation("ADD", a, b)
    gt = A.Operation("GREATER", a, b)
    for fr in ((0.5, 0.5, 0.5), (0.0, None, 0.5), (None, None, None), (0.5, None, 0.0), (1.0, 0.5, None)):
        ka, kb, kc = masks(rng, n, *fr)
        t3 = [(x, ka), (y, kb), (z, kc)]
        tf = [(x, ka), (y, kb), (flag, kc)]
        check(gx, A.Operation("ADD", add, c), t3, n, f"(a + b) + c validity {fr}")
        got, ok = check(gx, A.Operation("IS_NULL", add), t3, n, f"IS_NULL(a + b) {fr}", with_valid=True)
        va = np.ones(n, bool) if ka is None else ka
        vb = np.ones(n, bool) if kb is None else kb
        vc = np.ones(n, bool) if kc is None else kc
        assert ok.all() and np.array_equal(got, ~(va & vb))
        got, ok = check(gx, A.Operation("NULL_EQUAL", add, c), t3, n, f"NULL_EQUAL(a + b, c) {fr}", with_valid=True)
        assert ok.all() and np.array_equal(got, np.where(va & vb & vc, x + y == z, (va & vb) == vc))
        g = x > y
        got, ok = check(gx, A.Operation("NULL_LOGICAL_OR", gt, c), tf, n, f"NULL_LOGICAL_OR(a > b, c) {fr}", with_valid=True)
        assert np.array_equal(ok, (va & vb & vc) | (va & vb & g) | (vc & flag))
        assert np.array_equal(got[ok], ((va & vb & g) | (vc & flag))[ok])
        got, ok = check(gx, A.Operation("NULL_LOGICAL_AND", gt, c), tf, n, f"NULL_LOGICAL_AND(a > b, c) {fr}", with_valid=True)
        assert np.array_equal(ok, (va & vb & vc) | (va & vb & ~g) | (vc & ~flag))
    # an invalid literal makes every row null; IS_NULL of that is true and valid
    none = A.Literal(None, np.int32)
    got, ok = check(gx, A.Operation("MUL", a, none), [(x, None)], n, "a * null literal")
    assert not ok.any()
    got, ok = check(gx, A.Operation("IS_NULL", A.Operation("MUL", a, none)), [(x, None)], n, "IS_NULL(a * null literal)")
    assert ok.all() and got.all()
    # a null spilled to a slot and read back, on either side of the root
    ka, kb, kc, kd = masks(rng, n, 0.6, None, None, 0.7)
    t4 = [(x, ka), (y, kb), (z, kc), (w, kd)]
    got, ok = check(gx, A.Operation("SUB", add, A.Operation("MUL", c, d)), t4, n, "a null through a spill slot")
    assert np.array_equal(ok, ka & kd)
    check(gx, A.Operation("SUB", A.Operation("MUL", c, b), A.Operation("ADD", a, d)), t4, n, "nulls on the unspilled side")


def test_no_contraction_two_roundings(gx):
    """float64 a * b + c on 2000 standard-normal rows: a fused multiply-add differs from the two-rounding result on hundreds of these
    rows (counted here with exact rationals, so that the case cannot go vacuous); the kernel must give NumPy's a * b + c on all"""
    _, Column, ops, A = gx
    rng = np.random.default_rng(7)
    a, b, c = rng.standard_normal(2000), rng.standard_normal(2000), rng.standard_normal(2000)
    two = a * b + c
    differ = 0
    for x, y, z, t in zip(a.tolist(), b.tolist(), c.tolist(), two.tolist()):
        exact = Fraction(x) * Fraction(y) + Fraction(z)
        differ += float(exact) != t              # float(Fraction) rounds once, correctly: the fused result
    assert differ > 100, differ
    r = [A.ColumnReference(i) for i in range(3)]
    got = ops.compute_column([Column.from_numpy(v) for v in (a, b, c)], A.Operation("ADD", A.Operation("MUL", r[0], r[1]), r[2]))
    assert np.array_equal(bits_of(got.to_numpy()), bits_of(two))
    got = ops.compute_column([Column.from_numpy(v) for v in (a, b, c)], A.Operation("SUB", r[2], A.Operation("MUL", r[0], r[1])))
    assert np.array_equal(bits_of(got.to_numpy()), bits_of(c - a * b))


# ------------------------------------------------------------------------------------------------ DataFrame.eval / query
def test_dataframe_eval_and_query_against_pandas(gx):
    import pandas as pd
    cudf_amd, Column, ops, A = gx
    rng = np.random.default_rng(9)
    n = 5000
    pdf = pd.DataFrame({"a": rng.integers(-50, 50, n), "b": rng.integers(1, 9, n), "x": np.round(rng.normal(0, 5, n), 2),
                        "y": np.round(rng.normal(0, 5, n), 2) + 0.5, "f": rng.random(n) < 0.5, "g": rng.random(n) < 0.3})
    df = cudf_amd.DataFrame.from_pandas(pdf)
    for text in ("a * b + a", "x * y + x", "a + x", "x - a * 2", "2 - x", "a + 1", "1.5 * x", "x / y", "a / b", "a % b", "x % y",
                 "a > b", "x <= y", "a == b", "a != 3", "(a > b) & (x < 5)", "(a > b) | (x < y)", "~f", "f & g", "f | ~g",
                 "a > 0 and x < 1", "f or a < b", "not f", "not (a > b and f)", "(a + b) * (x + y)", "a + f", "a * a + b * b",
                 "x ** 2"):
        got = df.eval(text)
        want = pdf.eval(text, engine="python")
        assert got.null_count == 0 and got.dtype == want.dtype, (text, got.dtype, want.dtype)
        if want.dtype.kind == "f":
            np.testing.assert_allclose(got.to_numpy(), want.to_numpy(), rtol=1e-15, atol=0, equal_nan=True, err_msg=text)
        else:
            assert np.array_equal(got.to_numpy(), want.to_numpy()), text
    got = df.eval("a // b")                  # FLOOR_DIV is the AST's: floor(double / double) into FLOAT64
    assert got.dtype == np.float64 and np.array_equal(got.to_numpy(), np.floor(pdf["a"].to_numpy() / pdf["b"].to_numpy()))
    for text in ("a > b", "(a > b) & (x < y)", "f and x > 0 or a == 1", "not f", "x * y + x > 3"):
        got = df.query(text).to_pandas()
        want = pdf.query(text, engine="python").reset_index(drop=True)
        pd.testing.assert_frame_equal(got, want)
    for text in ("abs(a)", "a.b", "a[0]", "a ^ b", "a << 1", "a < b < 3", "a in b", "'s' + a", "-a", "a if f else b"):
        with pytest.raises(ValueError):
            df.eval(text)
    with pytest.raises(KeyError):
        df.eval("nope + 1")
    with pytest.raises(TypeError):
        df.eval("a + 1.5")
    with pytest.raises(ValueError):
        df.query("a + b")


# ------------------------------------------------------------------------------------------------ the C++ surface
def test_cpp_surface_cases():
    """cudf::compute_column on views made by cudf::slice, nullable and non-nullable results, every throw, ast::tree ownership"""
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "cudf_transform_tests")], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    runs = [l for l in r.stdout.splitlines() if l.startswith("[ OK ]")]
    assert len(runs) >= 14 and ", 0 failed" in r.stdout
