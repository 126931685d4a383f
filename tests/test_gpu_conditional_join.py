"""GPU: cudf::conditional_*_join -- gx_conditional_join_count / _write (cudf_amd/csrc/gx_conditional_join.hip), ops.conditional_*,
DataFrame.join_where and the C++ surface (tests/cpp/cudf_conditional_join_tests).
The main oracle is NumPy on the host: the predicate on the broadcast n_left x n_right grid (tests/conditional_join_model.py, with
the per-value rules of tests/expression_model.py), then np.nonzero -- already in (left, right) order, so gather maps compare bit
for bit.  A second arm for five pinned predicates materialises the grid on the device (ops.repeat / ops.tile, ops.compute_column,
ops.apply_boolean_mask: all held to NumPy by their own tests).  Calls through the C ABI place every bitmap at a begin bit, put guard
bytes behind both outputs, and compare the count pass's total with the rows written.  Row counts come from
gx_conditional_join_tile() and gx_conditional_join_pairs_per_run()."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import conditional_join_model as CJ
from tests import expression_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ["int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float32", "float64", "bool"]
CMPS = ["EQUAL", "NOT_EQUAL", "LESS", "GREATER", "LESS_EQUAL", "GREATER_EQUAL"]
KINDS = CJ.KINDS
BEGIN_BITS = (0, 1, 31, 33)
GUARD = 0x5A
NO_MATCH = CJ.NO_MATCH


@pytest.fixture(scope="module")
def gx():
    import cudf_amd
    from cudf_amd import Column, ops
    from cudf_amd import ast as A
    return cudf_amd, Column, ops, A


@pytest.fixture(scope="module")
def shape(gx):
    lib = gx[0]._lib.lib
    tl, tr = ctypes.c_int(0), ctypes.c_int(0)
    lib.gx_conditional_join_tile(ctypes.byref(tl), ctypes.byref(tr))
    return tl.value, tr.value, int(lib.gx_conditional_join_pairs_per_run()), int(lib.gx_conditional_join_grid_cap())


def col(v, valid=None):
    v = np.asarray(v)
    return v, (np.ones(len(v), dtype=bool) if valid is None else np.asarray(valid, dtype=bool))


def lits_of(literals):
    return [(np.zeros(1, dtype=l.dtype) if l.value is None else np.array([l.value], dtype=l.dtype), np.array([l.value is not None]))
            for l in literals]


def oracle(A, expr, left, right, kind):
    nodes, columns, literals = A.flatten_pair(expr)
    return CJ.join_of(CJ.grid_matches(nodes, columns, left, right, lits_of(literals)), kind)


def abi_join(gx, expr, left, right, kind, begin_bits=(0, 0), size_only=False):
    """The join through the C ABI on host arrays.  left / right: [(values, validity)] by table index; begin_bits = (left, right)
    places every bitmap of a side at that bit of a larger buffer.  Guard bytes behind both outputs; the count pass's total must
    equal the rows written.  Returns (left, right) or one array, and the total."""
    import torch
    cudf_amd, Column, ops, A = gx
    L = cudf_amd._lib
    nodes, columns, literals = A.flatten_pair(expr)
    sides = {"left": left, "right": right}
    n_left = len(left[0][0]) if left else 0
    n_right = len(right[0][0]) if right else 0
    keep, col_structs = [], []
    for table, index in columns:
        v, ok = sides[table][index]
        bb = begin_bits[table == "right"]
        data = torch.from_numpy(np.ascontiguousarray(v).view(np.uint8).copy()).cuda() if len(v) else torch.zeros(8, dtype=torch.uint8, device="cuda")
        mask_ptr = None
        if not ok.all() or bb:
            bits = np.zeros(bb + len(v) + 64, dtype=np.uint8)
            bits[:bb] = 1 - (np.arange(bb) % 2)                  # noise in front of the begin bit
            bits[bb:bb + len(v)] = ok
            bits[bb + len(v):] = 1
            mask = torch.from_numpy(np.packbits(bits, bitorder="little").copy()).cuda()
            keep.append(mask)
            mask_ptr = mask.data_ptr()
        keep.append(data)
        col_structs.append(L.ExprColumn(data.data_ptr(), mask_ptr, bb if mask_ptr else 0, M.GX[np.dtype(v.dtype)], int(table == "right")))
    scalars = [ops._device_scalar(l.value, l.dtype) for l in literals]
    node_arr = (L.ExprNode * len(nodes))(*[L.ExprNode(*nd) for nd in nodes])
    col_arr = (L.ExprColumn * max(len(col_structs), 1))(*col_structs)
    lit_arr = (L.ExprLiteral * max(len(literals), 1))(*[L.ExprLiteral(v.data_ptr(), b.data_ptr(), M.GX[np.dtype(l.dtype)], 0)
                                                        for l, (v, b) in zip(literals, scalars)])
    k = KINDS.index(kind)
    head = (node_arr, len(nodes), col_arr, len(col_structs), lit_arr, len(literals), n_left, n_right, k)
    lib = L.lib
    nbytes = ctypes.c_size_t(0)
    assert lib.gx_conditional_join_count(*head, None, None, ctypes.byref(nbytes), None) == 0
    tmp = torch.empty(nbytes.value + 64, dtype=torch.uint8, device="cuda")
    tmp[nbytes.value:] = GUARD
    sizes = torch.full((3,), -1, dtype=torch.int64, device="cuda")
    stream = ops.stream_ptr()
    assert lib.gx_conditional_join_count(*head, sizes.data_ptr(), tmp.data_ptr(), ctypes.byref(nbytes), stream) == 0
    total, left_total, guard = (int(x) for x in sizes.tolist())
    assert guard == -1 and 0 <= left_total <= total
    if size_only:
        return None, total
    pairs = k <= 2
    outs = [torch.full((total * 4 + 64,), GUARD, dtype=torch.uint8, device="cuda") for _ in range(2 if pairs else 1)]
    rc = lib.gx_conditional_join_write(*head, total, left_total, tmp.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr() if pairs else None,
                                       stream)
    assert rc == 0, rc
    host = [o.cpu().numpy() for o in outs]
    for h in host:
        assert (h[total * 4:] == GUARD).all(), "bytes behind the last output row were written"
    assert (tmp[nbytes.value:].cpu().numpy() == GUARD).all(), "bytes behind the scratch were written"
    arrays = [h[:total * 4].view(np.int32).copy() for h in host]
    if pairs:
        assert not ((arrays[0] == 0x5A5A5A5A) & (arrays[1] == 0x5A5A5A5A)).any(), "an output row was not written"
    return (tuple(arrays) if pairs else arrays[0]), total


def same(got, want, what=""):
    if isinstance(want, tuple):
        for g, w, side in zip(got, want, ("left", "right")):
            same(g, w, f"{what} {side}")
        return
    assert got.dtype == np.int32 and got.shape == want.shape, (what, got.shape, want.shape)
    if not (got == want).all():
        i = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{what}: first difference at {i}: got {got[i]}, want {want[i]}")


def check(gx, expr, left, right, kinds=KINDS, begin_bits=(0, 0), what=""):
    A = gx[3]
    for kind in kinds:
        want = oracle(A, expr, left, right, kind)
        got, total = abi_join(gx, expr, left, right, kind, begin_bits)
        same(got, want, f"{what} {kind}")
        assert total == (len(want[0]) if isinstance(want, tuple) else len(want))


def refs(A):
    return (lambda i: A.ColumnReference(i, "left")), (lambda i: A.ColumnReference(i, "right"))


def values(rng, dt, n, span=6):
    dt = np.dtype(dt)
    if dt == np.bool_:
        return rng.integers(0, 2, n).astype(np.bool_)
    if dt.kind == "f":
        v = rng.integers(-span, span + 1, n).astype(dt) / 2
        if n >= 8:
            v[rng.permutation(n)[:6]] = [np.nan, np.inf, -np.inf, -0.0, 0.0, np.nan]
        return v
    lo = 0 if dt.kind == "u" else -span
    v = rng.integers(lo, span + 1, n).astype(dt)
    if n >= 4:
        info = np.iinfo(dt)
        v[rng.permutation(n)[:2]] = [info.min, info.max]
    return v


# ------------------------------------------------------------------------------------------------ row counts
@pytest.mark.parametrize("kind", KINDS)
def test_row_counts_every_kind(gx, shape, kind):
    """the row counts of the issue on both sides: tile, chunk and R edges, empty sides; a range predicate and a sparse equality"""
    A = gx[3]
    TL, TR, R, _ = shape
    l, r = refs(A)
    rng = np.random.default_rng(11)
    lt = A.Operation("LESS", l(0), r(0))
    eq = A.Operation("EQUAL", l(0), r(0))
    lefts = sorted({0, 1, 63, 64, 65, TL - 1, TL, TL + 1, 2 * TL + 3})
    rights = sorted({0, 1, R - 1, R, R + 1, TR - 1, TR, TR + 1, 3 * TR + 5})
    for nl in lefts:
        a = rng.integers(0, 900, nl).astype(np.int64)
        for nr in rights:
            b = rng.integers(0, 900, nr).astype(np.int64)
            check(gx, lt, [col(a)], [col(b)], kinds=(kind,), what=f"LESS {nl}x{nr}")
            check(gx, eq, [col(a)], [col(b)], kinds=(kind,), what=f"EQUAL {nl}x{nr}")


def test_capped_grid_second_trip(gx, shape):
    """more left tiles than the grid cap: a workgroup's second tile"""
    A = gx[3]
    TL, TR, R, cap = shape
    l, r = refs(A)
    nl, nr = cap * TL + TL + 1, 33
    rng = np.random.default_rng(12)
    a, b = rng.integers(0, 4000, nl).astype(np.int32), rng.integers(0, 4000, nr).astype(np.int32)
    expr = A.Operation("EQUAL", l(0), r(0))
    hit = a[:, None] == b[None, :]
    for kind in KINDS:
        got, total = abi_join(gx, expr, [col(a)], [col(b)], kind)
        same(got, CJ.join_of(hit, kind), kind)


def test_segments_of_several_chunks(gx, shape):
    """few left tiles against a long right table: the right table is cut into segments of several chunks each, one workgroup per
    (tile, segment); the pairs of a left row come out of several workgroups and still ascend"""
    A = gx[3]
    TL, TR, R, _ = shape
    l, r = refs(A)
    nl, nr = 2100, 1000 * TR + 3
    rng = np.random.default_rng(14)
    a = rng.integers(0, 3000, nl).astype(np.int32)
    a[5::97] = -1                                                # rows without a match
    b = rng.integers(0, 3000, nr).astype(np.int32)
    b[nr - 1] = 2999
    expr = A.Operation("EQUAL", l(0), r(0))
    wl, wr = [], []
    for s in range(0, nl, 256):
        i, j = np.nonzero(a[s:s + 256, None] == b[None, :])
        wl.append(i + s)
        wr.append(j)
    wl, wr = np.concatenate(wl).astype(np.int32), np.concatenate(wr).astype(np.int32)
    got, total = abi_join(gx, expr, [col(a)], [col(b)], "inner")
    same(got, (wl, wr), "inner")
    hit = np.zeros(nl, dtype=bool)
    hit[wl] = True
    (ll, lr), total = abi_join(gx, expr, [col(a)], [col(b)], "left")
    assert total == len(wl) + int((~hit).sum())
    keep = lr != NO_MATCH
    same(ll[keep], wl, "left join, matched rows")
    same(lr[keep], wr, "left join, right rows")
    same(ll[~keep], np.flatnonzero(~hit).astype(np.int32), "left join, unmatched rows")
    assert (np.diff(ll.astype(np.int64)) >= 0).all()
    semi, _ = abi_join(gx, expr, [col(a)], [col(b)], "leftsemi")
    anti, _ = abi_join(gx, expr, [col(a)], [col(b)], "leftanti")
    same(semi, np.flatnonzero(hit).astype(np.int32), "semi")
    same(anti, np.flatnonzero(~hit).astype(np.int32), "anti")
    (fl, fr), total = abi_join(gx, expr, [col(a)], [col(b)], "full")
    rhit = np.zeros(nr, dtype=bool)
    rhit[wr] = True
    same(fr[len(ll):], np.flatnonzero(~rhit).astype(np.int32), "full tail")
    same(fl[:len(ll)], ll, "full head")
    assert (fl[len(ll):] == NO_MATCH).all() and total == len(ll) + int((~rhit).sum())


def test_interval_join_16k_by_16k(gx):
    """l.lo <= r.t & r.t < l.hi at about 1e-3 selectivity, the oracle in row chunks"""
    A = gx[3]
    l, r = refs(A)
    n = 2**14
    rng = np.random.default_rng(13)
    lo = rng.integers(0, 10**6, n).astype(np.int64)
    hi = lo + rng.integers(0, 2001, n)
    t = rng.integers(0, 10**6, n).astype(np.int64)
    expr = A.Operation("LOGICAL_AND", A.Operation("LESS_EQUAL", l(0), r(0)), A.Operation("LESS", r(0), l(1)))
    wl, wr = [], []
    for s in range(0, n, 2048):
        m = (lo[s:s + 2048, None] <= t[None, :]) & (t[None, :] < hi[s:s + 2048, None])
        i, j = np.nonzero(m)
        wl.append(i + s)
        wr.append(j)
    want = (np.concatenate(wl).astype(np.int32), np.concatenate(wr).astype(np.int32))
    assert 0.3e-3 < len(want[0]) / n / n < 3e-3
    got, total = abi_join(gx, expr, [col(lo), col(hi)], [col(t)], "inner")
    same(got, want, "interval")
    assert total == len(want[0])


# ------------------------------------------------------------------------------------------------ predicates
@pytest.mark.parametrize("dt", DTYPES)
def test_six_comparisons(gx, dt):
    """every comparison on every dtype; floats carry NaN, +-0 and +-inf, integers their extremes"""
    A = gx[3]
    l, r = refs(A)
    rng = np.random.default_rng(DTYPES.index(dt))
    a, b = values(rng, dt, 67), values(rng, dt, 131)
    for op in CMPS:
        check(gx, A.Operation(op, l(0), r(0)), [col(a)], [col(b)], kinds=("inner", "full", "leftanti"), what=f"{op} {dt}")


def test_arithmetic_on_both_sides(gx):
    """l.a * 2 + 1 < r.b - l.c"""
    A = gx[3]
    l, r = refs(A)
    rng = np.random.default_rng(21)
    a, c, b = (rng.integers(-40, 40, n).astype(np.int32) for n in (130, 130, 261))
    expr = A.Operation("LESS", A.Operation("ADD", A.Operation("MUL", l(0), A.Literal(2, np.int32)), A.Literal(1, np.int32)),
                       A.Operation("SUB", r(0), l(1)))
    check(gx, expr, [col(a), col(c)], [col(b)], what="chain")


def balanced(A, leaves, depth):
    """a balanced tree of ADDs over 2^depth leaves, sides mixed: `depth - 1` spill slots"""
    level = leaves[:2**depth]
    while len(level) > 1:
        level = [A.Operation("ADD", level[i], level[i + 1]) for i in range(0, len(level), 2)]
    return level[0]


@pytest.mark.parametrize("slots", [1, 4])
def test_spill_slots_mix_sides(gx, slots):
    """balanced trees whose leaves alternate between the tables: one and four spill slots"""
    cudf_amd, Column, ops, A = gx
    L = cudf_amd._lib
    l, r = refs(A)
    rng = np.random.default_rng(22 + slots)
    nl, nr = 70, 135
    left = [col(rng.integers(-9, 10, nl).astype(np.int64)) for _ in range(4)]
    right = [col(rng.integers(-9, 10, nr).astype(np.int64), rng.random(nr) < 0.9) for _ in range(4)]
    leaf = [(l if i % 2 == 0 else r)(i // 2) for i in range(8)]          # 8 leaf objects: l0 r0 l1 r1 ...
    if slots == 1:
        tree = balanced(A, leaf, 2)
    else:   # two depth-3 trees over the same leaves (2 slots each), combined twice (3 slots), and those combined (4 slots): 27 nodes,
        # 63 instructions -- a full tree of 32 leaves, which as separate objects would be beyond the node limit
        half, other = balanced(A, leaf, 3), balanced(A, leaf[::-1], 3)
        tree = A.Operation("MUL", A.Operation("ADD", half, other), A.Operation("SUB", other, half))
    expr = A.Operation("GREATER", tree, A.Literal(3, np.int64))
    nodes, columns, literals = A.flatten_pair(expr)
    node_arr = (L.ExprNode * len(nodes))(*[L.ExprNode(*nd) for nd in nodes])
    cd = (ctypes.c_int32 * len(columns))(*[M.GX[np.dtype(np.int64)]] * len(columns))
    ld = (ctypes.c_int32 * 1)(M.GX[np.dtype(np.int64)])
    ins = (L.ExprInstr * 64)()
    n_ins, n_slots = ctypes.c_int(0), ctypes.c_int(0)
    assert L.lib.gx_expr_plan(node_arr, len(nodes), cd, len(columns), ld, 1, ins, 64, ctypes.byref(n_ins), ctypes.byref(n_slots)) == 0
    assert n_slots.value == slots
    check(gx, expr, left, right, what=f"{slots} slots")


def test_one_sided_and_literal_predicates(gx):
    """a predicate that reads only LEFT columns, one that reads only RIGHT columns, the literals true (the cross product) and false"""
    A = gx[3]
    l, r = refs(A)
    rng = np.random.default_rng(24)
    a, b = rng.integers(0, 5, 71).astype(np.int16), rng.integers(0, 5, 259).astype(np.int16)
    check(gx, A.Operation("GREATER", l(0), A.Literal(2, np.int16)), [col(a)], [col(b)], what="left only")
    check(gx, A.Operation("GREATER", r(0), A.Literal(2, np.int16)), [col(a)], [col(b)], what="right only")
    check(gx, A.Literal(True, np.bool_), [col(a)], [col(b)], what="true")
    check(gx, A.Literal(False, np.bool_), [col(a)], [col(b)], what="false")
    check(gx, A.Literal(None, np.bool_), [col(a)], [col(b)], what="null literal")


def test_heavy_programs_and_their_light_twins(gx):
    """l.a // r.b == 3 (FLOOR_DIV, non-zero r.b) and l.x / r.y > 0.5 run the HEAVY kernel; the same shapes with * run the light one"""
    A = gx[3]
    l, r = refs(A)
    rng = np.random.default_rng(25)
    a = rng.integers(-60, 60, 131).astype(np.int64)
    b = rng.integers(1, 12, 262).astype(np.int64) * rng.choice([-1, 1], 262)
    x, y = rng.standard_normal(131), rng.standard_normal(262)
    y[::17] = 0.0
    f64 = lambda v: A.Literal(v, np.float64)
    check(gx, A.Operation("EQUAL", A.Operation("FLOOR_DIV", l(0), r(0)), f64(3.0)), [col(a)], [col(b)], what="floor_div")
    check(gx, A.Operation("GREATER", A.Operation("TRUE_DIV", l(0), r(0)), f64(0.5)), [col(x)], [col(y)], what="true_div")
    check(gx, A.Operation("EQUAL", A.Operation("MUL", l(0), r(0)), A.Literal(36, np.int64)), [col(a)], [col(b)], what="mul int")
    check(gx, A.Operation("GREATER", A.Operation("MUL", l(0), r(0)), f64(0.5)), [col(x)], [col(y)], what="mul float")


def test_mixed_widths_through_casts(gx):
    """int8 on the left against int64 on the right"""
    A = gx[3]
    l, r = refs(A)
    rng = np.random.default_rng(26)
    a, b = rng.integers(-128, 128, 200).astype(np.int8), rng.integers(-130, 130, 300).astype(np.int64)
    check(gx, A.Operation("LESS_EQUAL", A.Operation("CAST_TO_INT64", l(0)), r(0)), [col(a)], [col(b)], what="cast")


# ------------------------------------------------------------------------------------------------ nulls
@pytest.mark.parametrize("bb", BEGIN_BITS)
@pytest.mark.parametrize("nullable", ["left", "right", "both"])
def test_nullable_columns_at_begin_bits(gx, shape, nullable, bb):
    """nullable columns on each side and on both, every bitmap at begin bit bb: a null result is no match"""
    A = gx[3]
    TL, TR, R, _ = shape
    l, r = refs(A)
    rng = np.random.default_rng(31 + bb)
    nl, nr = TL + 7, TR + R + 1
    a, b = rng.integers(0, 6, nl).astype(np.int32), rng.integers(0, 6, nr).astype(np.int32)
    av = rng.random(nl) < 0.7 if nullable in ("left", "both") else None
    bv = rng.random(nr) < 0.7 if nullable in ("right", "both") else None
    for op in ("EQUAL", "NULL_EQUAL", "LESS"):
        check(gx, A.Operation(op, l(0), r(0)), [col(a, av)], [col(b, bv)], begin_bits=(bb, (bb * 7) % 40), what=f"{op} {nullable} {bb}")


def test_null_aware_operators(gx):
    """IS_NULL(r.b); NULL_EQUAL matching null with null; Kleene NULL_LOGICAL_OR / AND"""
    A = gx[3]
    l, r = refs(A)
    rng = np.random.default_rng(32)
    nl, nr = 90, 150
    a, b = rng.integers(0, 3, nl).astype(np.int8), rng.integers(0, 3, nr).astype(np.int8)
    av, bv = rng.random(nl) < 0.6, rng.random(nr) < 0.6
    p, q = rng.integers(0, 2, nl).astype(np.bool_), rng.integers(0, 2, nr).astype(np.bool_)
    left, right = [col(a, av), col(p, av)], [col(b, bv), col(q, bv)]
    check(gx, A.Operation("IS_NULL", r(0)), left, right, what="is_null right")
    check(gx, A.Operation("LOGICAL_AND", A.Operation("IS_NULL", l(0)), A.Operation("NOT", A.Operation("IS_NULL", r(0)))), left, right,
          what="is_null both")
    check(gx, A.Operation("NULL_EQUAL", l(0), r(0)), left, right, what="null_equal")
    check(gx, A.Operation("NULL_LOGICAL_OR", l(1), r(1)), left, right, what="kleene or")
    check(gx, A.Operation("NULL_LOGICAL_AND", l(1), r(1)), left, right, what="kleene and")


def test_all_null_right_column(gx):
    """INNER is empty, LEFT is all NO_MATCH, ANTI is every row"""
    A = gx[3]
    l, r = refs(A)
    a, b = np.arange(300, dtype=np.int32), np.arange(77, dtype=np.int32)
    expr = A.Operation("GREATER_EQUAL", l(0), r(0))
    left, right = [col(a)], [col(b, np.zeros(77, dtype=bool))]
    (il, ir), _ = abi_join(gx, expr, left, right, "inner")
    assert len(il) == 0 and len(ir) == 0
    (ll, lr), _ = abi_join(gx, expr, left, right, "left")
    same(ll, a, "left rows")
    assert (lr == NO_MATCH).all()
    anti, _ = abi_join(gx, expr, left, right, "leftanti")
    same(anti, a, "anti")
    check(gx, expr, left, right, what="all null right")


# ------------------------------------------------------------------------------------------------ kind-specific cases
def test_left_rows_with_no_one_many_matches_at_tile_edges(gx, shape):
    A = gx[3]
    TL, TR, R, _ = shape
    l, r = refs(A)
    nl, nr = 2 * TL + 1, 2 * TR + 3
    a = np.full(nl, -1, dtype=np.int32)
    b = np.arange(nr, dtype=np.int32) % 7 + 100
    b[nr - 1] = 55
    for i, v in ((0, 100), (63, 55), (64, 101), (TL - 1, 102), (TL, 55), (TL + 1, 103), (2 * TL, 104)):   # 55: one match, the last right row
        a[i] = v
    check(gx, A.Operation("EQUAL", l(0), r(0)), [col(a)], [col(b)], what="tile edges")


@pytest.mark.parametrize("case", ["every", "none", "first", "last", "bit31", "bit32"])
def test_full_join_unmatched_right_rows(gx, shape, case):
    """FULL where every, no, and exactly one right row is unmatched: r = 0, r = n_right - 1, the word edges 31 / 32"""
    A = gx[3]
    TL, TR, R, _ = shape
    l, r = refs(A)
    nl, nr = 70, TR + 37
    b = np.arange(nr, dtype=np.int64)
    if case == "every":
        a = np.full(nl, -5, dtype=np.int64)
        expr = A.Operation("EQUAL", l(0), r(0))
    else:
        a = np.full(nl, {"none": -1, "first": 0, "last": nr - 1, "bit31": 31, "bit32": 32}[case], dtype=np.int64)
        expr = A.Operation("NOT_EQUAL", l(0), r(0))
    want = oracle(A, expr, [col(a)], [col(b)], "full")
    tail = want[1][want[0] == NO_MATCH]
    assert len(tail) == {"every": nr, "none": 0}.get(case, 1)
    check(gx, expr, [col(a)], [col(b)], kinds=("full", "left"), what=case)


def test_semi_and_anti_are_complements_and_early_exit_is_exact(gx, shape):
    """SEMI and ANTI partition the left rows; rows whose only match is the last right row (the early exit must not cut the walk
    short) beside rows that match at once (whole waves and whole tiles leave early)"""
    A = gx[3]
    TL, TR, R, _ = shape
    l, r = refs(A)
    nl, nr = 3 * TL + 5, 4 * TR + 2
    b = np.zeros(nr, dtype=np.int32)
    b[nr - 1] = 9
    a = np.zeros(nl, dtype=np.int32)           # matches right row 0: tile 0 leaves after the first chunk
    a[TL:2 * TL] = 9                           # tile 1: only the last right row
    a[2 * TL:2 * TL + 64] = 9                  # tile 2: one wave late, the others early
    a[2 * TL + 100] = 4                        # and one row without any match
    expr = A.Operation("EQUAL", l(0), r(0))
    semi, _ = abi_join(gx, expr, [col(a)], [col(b)], "leftsemi")
    anti, _ = abi_join(gx, expr, [col(a)], [col(b)], "leftanti")
    same(semi, np.flatnonzero(a != 4).astype(np.int32), "semi")
    same(anti, np.array([2 * TL + 100], dtype=np.int32), "anti")
    assert len(np.intersect1d(semi, anti)) == 0 and len(semi) + len(anti) == nl


# ------------------------------------------------------------------------------------------------ the device arm
@pytest.mark.parametrize("name", ["less", "interval", "floor_div", "null_equal", "kleene"])
def test_against_the_materialised_grid(gx, name):
    """the second oracle: repeat / tile the two tables to n_left * n_right rows, compute_column, apply_boolean_mask"""
    cudf_amd, Column, ops, A = gx
    rng = np.random.default_rng(41)
    nl, nr = 301, 517
    a = rng.integers(0, 50, nl).astype(np.int64)
    a2 = a + rng.integers(0, 5, nl)
    b = rng.integers(1, 50, nr).astype(np.int64)
    av, bv = rng.random(nl) < 0.8, rng.random(nr) < 0.8
    p, q = rng.integers(0, 2, nl).astype(np.bool_), rng.integers(0, 2, nr).astype(np.bool_)
    left = [Column.from_numpy(a, av), Column.from_numpy(a2), Column.from_numpy(p, av)]
    right = [Column.from_numpy(b, bv), Column.from_numpy(q, bv)]

    def pred(l, r):
        return {"less": lambda: A.Operation("LESS", l(0), r(0)),
                "interval": lambda: A.Operation("LOGICAL_AND", A.Operation("LESS_EQUAL", l(0), r(0)), A.Operation("LESS", r(0), l(1))),
                "floor_div": lambda: A.Operation("EQUAL", A.Operation("FLOOR_DIV", l(0), r(0)), A.Literal(3.0, np.float64)),
                "null_equal": lambda: A.Operation("NULL_EQUAL", l(0), r(0)),
                "kleene": lambda: A.Operation("NULL_LOGICAL_OR", l(2), r(1))}[name]()

    l, r = refs(A)
    got_l, got_r = ops.conditional_inner_join(left, right, pred(l, r))
    # the grid as one table: left columns repeated (each row n_right times), right columns tiled, then the row numbers
    li = Column.from_numpy(np.arange(nl, dtype=np.int32))
    ri = Column.from_numpy(np.arange(nr, dtype=np.int32))
    grid = [ops.repeat([c], nr)[0] for c in left] + [ops.tile([c], nl)[0] for c in right]
    gl, gr = ops.repeat([li], nr)[0], ops.tile([ri], nl)[0]
    one = lambda i: A.ColumnReference(i)
    mask = ops.compute_column(grid, pred(one, lambda i: one(len(left) + i)))
    want_l, want_r = ops.apply_boolean_mask([gl, gr], mask)
    same(got_l.to_numpy(), want_l.to_numpy(), "left")
    same(got_r.to_numpy(), want_r.to_numpy(), "right")
    assert got_l.size > 0


# ------------------------------------------------------------------------------------------------ overflow
def test_more_than_int32_max_pairs(gx):
    """46341^2 = 2 147 488 281 pairs: the size is exact in 64 bits, the join raises without allocating; 46340^2 fits (size only)"""
    cudf_amd, Column, ops, A = gx
    true = A.Literal(True, np.bool_)
    big = [Column.from_numpy(np.zeros(46341, dtype=np.int8))]
    assert ops.conditional_join_size("inner", big, big, true) == 2_147_488_281
    with pytest.raises(OverflowError):
        ops.conditional_inner_join(big, big, true)
    fit = [Column.from_numpy(np.zeros(46340, dtype=np.int8))]
    assert ops.conditional_join_size("inner", fit, fit, true) == 2_147_395_600


def test_write_refuses_an_overflowing_total_before_it_launches(gx):
    L = gx[0]._lib
    node = (L.ExprNode * 1)(L.ExprNode(L.EXPR_LITERAL, 0, 0, 0))
    lit = (L.ExprLiteral * 1)(L.ExprLiteral(0x1000, None, L.BOOL8, 0))
    colz = (L.ExprColumn * 1)()
    rc = L.lib.gx_conditional_join_write(node, 1, colz, 0, lit, 1, 46341, 46341, 0, 2_147_488_281, 2_147_488_281, 0x1000, 0x1000, 0x1000, None)
    assert rc == -5    # GX_EOVERFLOW; the pointers are fake: nothing may be launched


# ------------------------------------------------------------------------------------------------ ops and DataFrame
def test_ops_entry_points_and_sizes(gx):
    cudf_amd, Column, ops, A = gx
    l, r = refs(A)
    rng = np.random.default_rng(51)
    a, b = rng.integers(0, 30, 400).astype(np.int32), rng.integers(0, 30, 333).astype(np.int32)
    av = rng.random(400) < 0.9
    left, right = [Column.from_numpy(a, av)], [Column.from_numpy(b)]
    expr = A.Operation("EQUAL", l(0), r(0))
    fns = {"inner": ops.conditional_inner_join, "left": ops.conditional_left_join, "full": ops.conditional_full_join,
           "leftsemi": ops.conditional_left_semi_join, "leftanti": ops.conditional_left_anti_join}
    for kind, fn in fns.items():
        want = oracle(A, expr, [col(a, av)], [col(b)], kind)
        got = fn(left, right, expr)
        got = tuple(g.to_numpy() for g in got) if isinstance(got, tuple) else got.to_numpy()
        same(got, want, kind)
        assert ops.conditional_join_size(kind, left, right, expr) == (len(want[0]) if isinstance(want, tuple) else len(want))
    with pytest.raises(TypeError):
        ops.conditional_inner_join(left, right, A.Operation("ADD", l(0), r(0)))
    with pytest.raises(IndexError):
        ops.conditional_inner_join(left, right, A.Operation("EQUAL", l(0), r(1)))
    with pytest.raises(ValueError):
        ops.conditional_join_size("cross", left, right, expr)
    with pytest.raises(ValueError):
        ops.compute_column(left, A.Operation("EQUAL", l(0), r(0)))


def test_join_where_against_pandas(gx):
    pd = pytest.importorskip("pandas")
    cudf_amd, Column, ops, A = gx
    from cudf_amd.dataframe import DataFrame
    rng = np.random.default_rng(52)
    lp = pd.DataFrame({"k": rng.integers(0, 40, 150), "lo": rng.integers(0, 100, 150), "w": rng.random(150)})
    lp["hi"] = lp["lo"] + rng.integers(0, 20, 150)
    rp = pd.DataFrame({"k": rng.integers(0, 40, 170), "t": rng.integers(0, 120, 170)})
    got = DataFrame.from_pandas(lp).join_where(DataFrame.from_pandas(rp), "lo <= t and t < hi and left.k != right.k").to_pandas()
    want = lp.merge(rp, how="cross").query("lo <= t and t < hi and k_x != k_y").reset_index(drop=True)
    assert list(got.columns) == ["k_x", "lo", "w", "hi", "k_y", "t"]
    pd.testing.assert_frame_equal(got, want[list(got.columns)], check_dtype=False)
    assert len(got) > 0


def test_join_where_kinds_names_and_errors(gx):
    cudf_amd, Column, ops, A = gx
    from cudf_amd.dataframe import DataFrame
    left = DataFrame({"a": np.array([1, 5, 9], dtype=np.int64), "v": np.array([10., 20., 30.])})
    right = DataFrame({"b": np.array([4, 6], dtype=np.int64), "v": np.array([1., 2.])})
    out = left.join_where(right, "a < b", how="left")
    assert out.columns == ["a", "v_x", "b", "v_y"]
    np.testing.assert_array_equal(out["a"].to_numpy(), [1, 1, 5, 9])
    np.testing.assert_array_equal(out["b"].valid_numpy(), [True, True, True, False])
    np.testing.assert_array_equal(out["b"].to_numpy()[:3], [4, 6, 6])
    out = left.join_where(right, "a > b and left.v > 25", how="outer")
    np.testing.assert_array_equal(out["a"].valid_numpy(), [True, True, True, True])
    np.testing.assert_array_equal(out["a"].to_numpy()[:4], [1, 5, 9, 9])
    np.testing.assert_array_equal(out["b"].valid_numpy(), [False, False, True, True])
    np.testing.assert_array_equal(out["b"].to_numpy()[2:], [4, 6])
    out = left.join_where(right, "a == b + 1", how="outer")     # 5 == 4 + 1: rows (1, 0); then left 0, 2 unmatched in place; right 1 last
    np.testing.assert_array_equal(out["a"].valid_numpy(), [True, True, True, False])
    np.testing.assert_array_equal(out["b"].valid_numpy(), [False, True, False, True])
    np.testing.assert_array_equal(out["v_y"].to_numpy()[[1, 3]], [1., 2.])
    semi = left.join_where(right, "a < b", how="leftsemi")
    anti = left.join_where(right, "a < b", how="leftanti")
    assert semi.columns == ["a", "v"] and list(semi["a"].to_numpy()) == [1, 5] and list(anti["a"].to_numpy()) == [9]
    expr = A.Operation("LESS", A.ColumnReference(0, "left"), A.ColumnReference(0, "right"))
    assert list(left.join_where(right, expr)["b"].to_numpy()) == [4, 6, 6]
    with pytest.raises(ValueError, match="both frames"):
        left.join_where(right, "v > 1")
    with pytest.raises(ValueError, match="not a bool"):
        left.join_where(right, "a + b")
    with pytest.raises(ValueError, match="how"):
        left.join_where(right, "a < b", how="right")
    with pytest.raises(KeyError):
        left.join_where(right, "a < nothing")


# ------------------------------------------------------------------------------------------------ the C++ surface
def test_cpp_conditional_join_binary(gx):
    binary = os.path.join(ROOT, "tests", "cpp", "cudf_conditional_join_tests")
    assert os.path.exists(binary), "run build() first"
    res = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and ", 0 failed" in res.stdout, res.stdout[-3000:] + res.stderr[-2000:]
