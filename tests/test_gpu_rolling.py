"""GPU: cudf::rolling_window / grouped_rolling_window -- ops.rolling_window, DataFrame.rolling and gx_rolling_window under them
(cudf_amd/csrc/gx_rolling.hip).  The reference is a plain loop over every row's cut window, written here: NumPy on the slice,
math.fsum for float sums.  Integer results, counts, MIN / MAX and the null masks are compared bit-exactly (== where a zero's sign
is unspecified); float SUM / MEAN are bounded by |got - exact| <= L * 2^-53 * sum|x_window| (the error of adding at most L terms
in ANY order), plus half a float ulp of the exact value for FLOAT32 output; MEAN: the bound over the count, plus one ulp.
Row counts come from gx_rolling_tile_rows() = T and gx_rolling_max_span() = S.  Every fixed window runs pinned to the tile kernel
(gx_rolling_set_kernel(1)) and to the row loop (2); both must match the reference, and each other where results are exact."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ("sum", "min", "max", "mean", "count_valid", "count_all")
DTYPES = ["int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float32", "float64", "bool"]
DEEP = ["int64", "int8", "float32", "float64"]
SIZES = {"1": lambda T: 1, "2": lambda T: 2, "63": lambda T: 63, "64": lambda T: 64, "65": lambda T: 65, "T-1": lambda T: T - 1,
         "T": lambda T: T, "T+1": lambda T: T + 1, "2T+3": lambda T: 2 * T + 3, "5T+17": lambda T: 5 * T + 17}


@pytest.fixture(scope="module")
def gx():
    import cudf_amd
    from cudf_amd import Column, ops
    yield cudf_amd, Column, ops
    cudf_amd._lib.lib.gx_rolling_set_kernel(0)


@pytest.fixture(scope="module")
def TS(gx):
    lib = gx[0]._lib.lib
    return int(lib.gx_rolling_tile_rows()), int(lib.gx_rolling_max_span())


def windows(n, S):
    """(preceding, following): the short ones, the empty ones, the whole column, halo exactly S (tile kernel) and S + 1 (row loop)"""
    return [(1, 0), (2, 0), (3, 2), (1, 1), (0, 3), (4, -1), (-2, 5), (n + 5, n + 5), (2, -3), (S // 2 + 1, S - S // 2), (S // 2 + 2, S - S // 2)]


# ------------------------------------------------------------------------------------------------ the reference
def _out_dtype(dt, op):
    dt = np.dtype(dt)
    if op in ("count_valid", "count_all"):
        return np.dtype(np.int32)
    if op == "mean":
        return np.dtype(np.float64)
    if op == "sum" and dt.kind != "f":
        return np.dtype(np.uint64 if dt == np.uint64 else np.int64)
    return dt


def _exact_sum(w):
    """the window's sum: exact (math.fsum) for finite values; inf and NaN as plain addition gives them"""
    if not np.all(np.isfinite(w)):
        if np.any(np.isnan(w)) or (np.any(w == np.inf) and np.any(w == -np.inf)):
            return math.nan
        return math.inf if np.any(w == np.inf) else -math.inf
    return math.fsum(w)


def reference(x, valid, p, f, gs=None, ge=None):
    """per row of x: the cut window [lo, hi] looped over.  Returns size, cnt, and per op the value arrays (None entries never read);
    float columns: "sum" is the EXACT sum as float64 and "abs" the sum of magnitudes, for the bound"""
    n = len(x)
    i = np.arange(n, dtype=np.int64)
    gs = np.zeros(n, np.int64) if gs is None else gs
    ge = np.full(n, n, np.int64) if ge is None else ge
    lo = np.maximum(i - np.asarray(p, np.int64) + 1, gs)
    hi = np.minimum(i + np.asarray(f, np.int64), ge - 1)
    size = np.maximum(hi - lo + 1, 0)
    is_f = x.dtype.kind == "f"
    xs = x.astype(np.float64) if is_f else (x if x.dtype == np.uint64 else x.astype(np.int64))
    cnt = np.zeros(n, np.int64)
    s = np.zeros(n, np.float64 if is_f else xs.dtype)
    ab = np.zeros(n, np.float64)
    mn, mx = np.zeros(n, x.dtype), np.zeros(n, x.dtype)
    memo = {}
    for r in range(n):
        if size[r] == 0:
            continue
        key = (int(lo[r]), int(hi[r]))
        got = memo.get(key)
        if got is None:
            w = xs[key[0]:key[1] + 1]
            wx = x[key[0]:key[1] + 1]
            if valid is not None:
                m = valid[key[0]:key[1] + 1]
                w, wx = w[m], wx[m]
            if len(w) == 0:
                got = (0, 0, 0.0, 0, 0)
            elif is_f:
                nan = np.isnan(wx)
                lo_v = wx[~nan].min() if not nan.all() else wx[0]
                hi_v = wx[nan][0] if nan.any() else wx.max()
                got = (len(w), _exact_sum(w), float(np.abs(w).sum()), lo_v, hi_v)
            else:
                with np.errstate(over="ignore"):
                    got = (len(w), w.sum(dtype=xs.dtype), 0.0, wx.min(), wx.max())
            if size[r] > 64:
                memo[key] = got
        cnt[r], s[r], ab[r], mn[r], mx[r] = got
    return {"size": size, "cnt": cnt, "sum": s, "abs": ab, "min": mn, "max": mx, "L": np.maximum(np.asarray(p, np.int64) + np.asarray(f, np.int64), 0)}


def _binade(y, bits):
    """one ulp of a `bits`-bit significand at y (the binade that holds |y|)"""
    if y == 0 or not math.isfinite(y):
        return 0.0
    return math.ldexp(1.0, math.frexp(abs(y))[1] - bits)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))
    return bool(np.array_equal(a, b))


def check(ref, dt, op, mp, got, got_valid, what):
    """one GPU result against the reference"""
    dt = np.dtype(dt)
    size, cnt = ref["size"], ref["cnt"]
    want_valid = size >= mp if op in ("count_valid", "count_all") else cnt >= max(mp, 1)
    assert got.dtype == _out_dtype(dt, op), what
    assert np.array_equal(got_valid, want_valid), (what, "validity", np.flatnonzero(got_valid != want_valid)[:8])
    v = want_valid
    if op == "count_valid":
        assert np.array_equal(got[v], cnt[v].astype(np.int32)), what
    elif op == "count_all":
        assert np.array_equal(got[v], size[v].astype(np.int32)), what
    elif op in ("min", "max"):
        assert _same(got[v], ref[op][v]), (what, np.flatnonzero(v)[:4], got[v][:4], ref[op][v][:4])
    elif dt.kind != "f":
        if op == "sum":
            assert np.array_equal(got[v], ref["sum"][v]), (what, got[v][:4], ref["sum"][v][:4])
        else:   # integers are summed exactly in 64 bits, then divided: the same two IEEE operations here
            want = ref["sum"][v].astype(np.float64) / cnt[v].astype(np.float64)
            assert np.array_equal(got[v], want), (what, got[v][:4], want[:4])
    else:
        exact, ab, L = ref["sum"][v], ref["abs"][v], np.broadcast_to(ref["L"], size.shape)[v].astype(np.float64)
        g, c = got[v].astype(np.float64), cnt[v].astype(np.float64)
        fin = np.isfinite(exact)
        assert np.array_equal(np.isnan(g), np.isnan(exact)), (what, "NaN rows")
        inf = np.isinf(exact)
        assert np.array_equal(g[inf], exact[inf]), (what, "inf rows")
        bound = L * 2.0**-53 * ab
        if op == "sum":
            if dt == np.float32:
                bound = bound + np.array([0.5 * _binade(y, 24) for y in exact])
            err = np.abs(g - exact)
        else:
            mean = np.where(fin, exact, 0.0) / c
            bound = bound / c + np.array([_binade(y, 53) for y in mean])
            err = np.abs(g - mean)
        bad = fin & ~(err <= bound)
        assert not bad.any(), (what, np.flatnonzero(bad)[:4], err[bad][:4], bound[bad][:4])


def run_gpu(gx, col, p, f, mp, op, kernel=0, keys=None):
    cudf_amd, Column, ops = gx
    cudf_amd._lib.lib.gx_rolling_set_kernel(kernel)
    try:
        out = ops.rolling_window(col, p, f, mp, op, group_keys=keys)
    finally:
        cudf_amd._lib.lib.gx_rolling_set_kernel(0)
    valid = out.valid_numpy()
    assert (valid is None) == (out.null_count == 0)
    if valid is None:
        valid = np.ones(out.size, bool)
    assert out.null_count == int((~valid).sum())
    return out.to_numpy(), valid


def make_column(dt, n, seed):
    rng = np.random.default_rng(seed)
    dt = np.dtype(dt)
    if dt.kind == "f":
        return ((rng.random(n) - 0.5) * 2000).astype(dt)
    if dt.kind == "b":
        return rng.random(n) < 0.5
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)      # full range: int64 sums wrap


def sweep(gx, x, valid, wins, mps_of, ops_list=OPS, keys=None, gs=None, ge=None, kernels=(1, 2)):
    _, Column, _ = gx
    col = Column.from_numpy(x, valid)
    key_cols = None if keys is None else [Column.from_numpy(k, kv) for k, kv in keys]
    for p, f in wins:
        ref = reference(x, valid, p, f, gs, ge)
        for op in ops_list:
            for mp in mps_of(p + f):
                res = []
                for kern in kernels:
                    got, gv = run_gpu(gx, col, p, f, mp, op, kern, key_cols)
                    check(ref, x.dtype, op, mp, got, gv, (len(x), str(x.dtype), p, f, op, mp, kern))
                    res.append((got, gv))
                if len(res) == 2 and not (x.dtype.kind == "f" and op in ("sum", "mean")):
                    assert np.array_equal(res[0][1], res[1][1]) and _same(res[0][0][res[0][1]], res[1][0][res[1][1]])


def _mps(L):
    return sorted({0, 1, 3, max(L, 0)})


# ------------------------------------------------------------------------------------------------ fixed windows
@pytest.mark.parametrize("dtype", DEEP)
@pytest.mark.parametrize("size", list(SIZES))
def test_fixed_windows_both_kernels(gx, TS, size, dtype):
    """every window of the list x six ops x min_periods {0, 1, 3, L}, pinned to each kernel, on a column without nulls"""
    T, S = TS
    n = SIZES[size](T)
    x = make_column(dtype, n, 100 + n)
    sweep(gx, x, None, windows(n, S), _mps)


def test_default_choice_switches_at_the_span_limit(gx, TS):
    """halo S takes the tile kernel by default, halo S + 1 the row loop -- and so does a window of a few rows, which the row loop
    serves faster (rolling windows): all equal the reference (and float sums equal, bit for bit, the kernel they are
    pinned to -- which is how the choice is seen)"""
    T, S = TS
    n = 2 * T + 3
    x = make_column("float64", n, 7)
    _, Column, _ = gx
    col = Column.from_numpy(x)
    for (p, f), kern in (((S // 2 + 1, S - S // 2), 1), ((S // 2 + 2, S - S // 2), 2), ((33, 31), 1), ((3, 2), 2)):
        d, dv = run_gpu(gx, col, p, f, 1, "sum", 0)
        k, kv = run_gpu(gx, col, p, f, 1, "sum", kern)
        assert np.array_equal(d, k) and np.array_equal(dv, kv)
        check(reference(x, None, p, f), x.dtype, "sum", 1, d, dv, (p, f))
    # the two kernels add in different orders: on this column their float sums are NOT all bit-equal, so the check above means something
    a, _ = run_gpu(gx, col, S // 2 + 1, S - S // 2, 1, "sum", 1)
    b, _ = run_gpu(gx, col, S // 2 + 1, S - S // 2, 1, "sum", 2)
    assert not np.array_equal(a, b)


def test_empty_windows_are_null_and_counts_are_valid_zeros_only_at_min_periods_0(gx, TS):
    T, _ = TS
    _, Column, _ = gx
    for n in (1, 65, T + 1):
        x = make_column("int64", n, 3)
        col = Column.from_numpy(x)
        for p, f in ((2, -3), (0, 0), (-4, 2), (1, -1)):
            for kern in (0, 1, 2):
                for op in ("sum", "min", "max", "mean"):
                    for mp in (0, 1):
                        _, gv = run_gpu(gx, col, p, f, mp, op, kern)
                        assert not gv.any()
                for op in ("count_valid", "count_all"):
                    got, gv = run_gpu(gx, col, p, f, 0, op, kern)
                    assert gv.all() and not got.any()
                    _, gv = run_gpu(gx, col, p, f, 1, op, kern)
                    assert not gv.any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_dtypes_all_ops(gx, TS, dtype):
    T, S = TS
    n = T + 65
    x = make_column(dtype, n, 11)
    valid = np.random.default_rng(12).random(n) < 0.8
    sweep(gx, x, None, [(3, 2), (S // 2 + 1, S - S // 2)], lambda L: (1,))
    sweep(gx, x, valid, [(3, 2), (70, 0)], lambda L: (0, 3))


@pytest.mark.parametrize("dtype", DEEP)
@pytest.mark.parametrize("size", ["65", "T+1", "2T+3"])
def test_nullable_input(gx, TS, size, dtype):
    """validity 0.8 and all-null: a null is the identity, never read, and a window without a valid value is null"""
    T, S = TS
    n = SIZES[size](T)
    rng = np.random.default_rng(n)
    x = make_column(dtype, n, 200 + n)
    valid = rng.random(n) < 0.8
    if np.dtype(dtype).kind == "f":
        x[~valid] = np.nan                         # a null's bytes must not leak: NaN would poison every sum
    sweep(gx, x, valid, windows(n, S), _mps)
    sweep(gx, x, np.zeros(n, bool), [(3, 2), (n + 5, n + 5), (S // 2 + 1, S - S // 2)], lambda L: (0, 1))


def test_sliced_view_with_an_unaligned_begin_bit(gx, TS):
    """the C ABI on rows [off, off + n) of a bigger column, the bitmap read from bit `off` (not a multiple of 32)"""
    cudf_amd, Column, ops = gx
    L, lib = cudf_amd._lib, cudf_amd._lib.lib
    from cudf_amd.column import ptr, stream_ptr
    import torch
    T, S = TS
    off, n = 45, T + 70
    x = make_column("int32", off + n + 9, 5)
    valid = np.random.default_rng(6).random(len(x)) < 0.7
    big = Column.from_numpy(x, valid)
    for kern in (1, 2):
        for p, f, op, name in ((3, 2, L.OP_SUM, "sum"), (40, 60, L.OP_MIN, "min"), (2, 0, L.OP_COUNT_VALID, "count_valid")):
            out = Column.empty(_out_dtype(x.dtype, name), n, nullable=True)
            nulls = torch.zeros(1, dtype=torch.int64, device="cuda")
            lib.gx_rolling_set_kernel(kern)
            rc = lib.gx_rolling_window(big.gx, ctypes.c_void_p(big.data.data_ptr() + 4 * off), big.mask_ptr, off, n, p, f, None, None, None, None,
                                       2, op, out.data_ptr, out.mask_ptr, ptr(nulls), stream_ptr())
            lib.gx_rolling_set_kernel(0)
            assert rc == 0
            gv = out.valid_numpy()
            assert int(nulls.item()) == int((~gv).sum())
            check(reference(x[off:off + n], valid[off:off + n], p, f), x.dtype, name, 2, out.to_numpy(), gv, (kern, p, f, name))


# ------------------------------------------------------------------------------------------------ float column classes
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_float_column_classes(gx, TS, dtype):
    T, S = TS
    n = T + 130
    rng = np.random.default_rng(21)
    wins = [(3, 2), (33, 31), (S // 2 + 1, S - S // 2)]
    big = 1e30 if dtype == "float32" else 1e200
    # large alternating-sign values: a prefix-difference scheme would lose every small term
    alt = (big * (1 + rng.random(n)) * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)).astype(dtype)
    alt[::7] = rng.random(len(alt[::7])).astype(dtype)
    sweep(gx, alt, None, wins, lambda L: (1,), ("sum", "mean", "min", "max"))
    # a single +inf: only the windows that hold it are inf, the others stay finite and inside the bound
    one = ((rng.random(n) - 0.5) * 100).astype(dtype)
    one[n // 3] = np.inf
    sweep(gx, one, None, wins, lambda L: (1,), ("sum", "mean", "max"))
    for p, f in wins:
        ref = reference(one, None, p, f)
        holds = (np.arange(n) - p + 1 <= n // 3) & (np.arange(n) + f >= n // 3)
        assert np.array_equal(np.isinf(ref["sum"]), holds) and 0 < holds.sum() < n
    # +inf and -inf L/2 rows apart: exactly the windows that hold both are NaN
    for p, f in wins:
        L = p + f
        two = ((rng.random(n) - 0.5) * 100).astype(dtype)
        a = n // 2
        two[a], two[a + L // 2] = np.inf, -np.inf
        sweep(gx, two, None, [(p, f)], lambda L: (1,), ("sum", "mean"))
        ref = reference(two, None, p, f)
        i = np.arange(n)
        both = (i - p + 1 <= a) & (i + f >= a + L // 2)
        assert np.array_equal(np.isnan(ref["sum"]), both) and both.any()
    # NaN payloads (quiet, signalling-looking, negative) and +-0 for MIN / MAX
    u = np.uint32 if dtype == "float32" else np.uint64
    pay = ((rng.random(n) - 0.5) * 10).astype(dtype)
    nan_bits = [0x7FC00001, 0xFFC00123, 0x7F800001] if dtype == "float32" else [0x7FF8000000000001, 0xFFF8000000000123, 0x7FF0000000000001]
    pay.view(u)[rng.choice(n, 40, replace=False)] = np.array(nan_bits, u)[rng.integers(0, 3, 40)]
    zeros = np.where(rng.random(n) < 0.5, 0.0, -0.0).astype(dtype)
    zeros[::5] = ((rng.random(len(zeros[::5])) - 0.5)).astype(dtype)
    valid = rng.random(n) < 0.8
    for col in (pay, zeros):
        sweep(gx, col, None, wins, lambda L: (1,), ("min", "max", "sum"))
        sweep(gx, col, valid, wins[:2], lambda L: (2,), ("min", "max"))


# ------------------------------------------------------------------------------------------------ groups
def _group_layouts(n, T, L):
    yield "ones", np.arange(n + 1)
    yield "one", np.array([0, n])
    sizes, cuts = [1, 2, max(L - 1, 1), L, L + 1], [0]
    k = 0
    while cuts[-1] < n:
        cuts.append(min(cuts[-1] + sizes[k % len(sizes)], n))
        k += 1
    yield "mixed", np.array(cuts)
    if n > 3 * T + 10:
        yield "tile_edges", np.array([0, 5, T, T + 7, 2 * T - 3, 5 * T + 9, n])    # a boundary on a tile boundary, a group over three tiles


def _keys_for(cuts, n, nkeys, rng):
    """key columns whose runs of equal rows are exactly the groups; nulls (equal to nulls) and mixed types"""
    g = np.repeat(np.arange(len(cuts) - 1), np.diff(cuts))
    if nkeys == 1:
        v = (g % 3 != 2)                                    # every third group's key is null, its bytes vary
        k = np.where(v, g * 7, rng.integers(0, 1000, n)).astype(np.int64)
        return [(k, v)]
    k0 = (g // 4).astype(np.int8)
    k1v = (g // 2) % 2 == 0
    k1 = np.where(k1v, (g // 2).astype(np.float64) * 0.5, rng.random(n))
    k2 = (g % 2).astype(np.uint16)
    return [(k0, None), (k1, k1v), (k2, None)]


@pytest.mark.parametrize("nkeys", [1, 3])
@pytest.mark.parametrize("dtype", ["int64", "float64"])
def test_grouped_windows(gx, TS, dtype, nkeys):
    T, S = TS
    rng = np.random.default_rng(31)
    for n, wins, valids in ((T + 70, [(3, 2), (1, 1), (4, -1), (-2, 5), (9, 8)], (False, True)),
                            (5 * T + 17, [(3, 2), (S // 2 + 1, S - S // 2)], (True,))):
        x = make_column(dtype, n, 40 + n)
        valid = rng.random(n) < 0.8
        if dtype == "float64":
            x[~valid] = np.nan
        for p, f in wins:
            for name, cuts in _group_layouts(n, T, p + f):
                gs = np.repeat(cuts[:-1], np.diff(cuts)).astype(np.int64)
                ge = np.repeat(cuts[1:], np.diff(cuts)).astype(np.int64)
                keys = _keys_for(cuts, n, nkeys, rng)
                for with_nulls in valids:
                    if dtype == "float64" and not with_nulls:
                        continue                             # the NaNs under the nulls would be values
                    sweep(gx, x, valid if with_nulls else None, [(p, f)], lambda L: (1, 3), ("sum", "max", "count_all", "mean"),
                          keys=keys, gs=gs, ge=ge)


# ------------------------------------------------------------------------------------------------ one window per row
def test_per_row_window_columns(gx, TS):
    T, S = TS
    _, Column, ops = gx
    rng = np.random.default_rng(51)
    for n in (65, T + 1, 2 * T + 3):
        for dtype in ("int64", "float64"):
            x = make_column(dtype, n, n)
            valid = rng.random(n) < 0.8
            if dtype == "float64":
                x[~valid] = np.nan
            pw, fw = rng.integers(-3, 41, n).astype(np.int32), rng.integers(-3, 41, n).astype(np.int32)
            ref = reference(x, valid, pw, fw)
            ref["L"] = np.maximum(ref["size"], 1)           # the terms a row's sum really has
            col = Column.from_numpy(x, valid)
            pc, fc = Column.from_numpy(pw), Column.from_numpy(fw)
            for op in OPS:
                for mp in (0, 1, 3):
                    got, gv = run_gpu(gx, col, pc, fc, mp, op)
                    check(ref, x.dtype, op, mp, got, gv, (n, dtype, op, mp))
            # a constant column is the fixed window: the same output as the row loop's, bit for bit
            cp, cf = Column.from_numpy(np.full(n, 3, np.int32)), Column.from_numpy(np.full(n, 2, np.int32))
            for op in OPS:
                a, av = run_gpu(gx, col, cp, cf, 1, op)
                b, bv = run_gpu(gx, col, 3, 2, 1, op, 2)
                assert np.array_equal(av, bv) and _same(a[av], b[bv])
                check(reference(x, valid, 3, 2), x.dtype, op, 1, a, av, (n, dtype, op, "constant"))


# ------------------------------------------------------------------------------------------------ the big column
def test_big_column(gx, TS):
    """2^22 + 4097 rows, window (3, 2) and the span limit, int64: the reference adds the window's rows offset by offset (one NumPy
    pass per offset), the validity and the counts come from the same passes"""
    T, S = TS
    n = 2**22 + 4097
    _, Column, _ = gx
    x = make_column("int64", n, 77)
    valid = np.random.default_rng(78).random(n) < 0.9
    col = Column.from_numpy(x, valid)
    for p, f, kerns in ((3, 2, (1, 2)), (S // 2 + 1, S - S // 2, (1,))):
        s, cnt = np.zeros(n, np.int64), np.zeros(n, np.int64)
        xv = np.where(valid, x, 0)
        if p + f <= 8:
            for d in range(-(p - 1), f + 1):
                src = slice(max(d, 0), n + min(d, 0))
                dst = slice(max(-d, 0), n - max(d, 0))
                with np.errstate(over="ignore"):
                    s[dst] += xv[src]
                cnt[dst] += valid[src]
        else:   # wide window: wrapping int64 prefix sums are exact mod 2^64 (this is the reference, not the kernel)
            with np.errstate(over="ignore"):
                cs = np.concatenate([[0], np.cumsum(xv)])
            cc = np.concatenate([[0], np.cumsum(valid)])
            i = np.arange(n)
            lo, hi = np.maximum(i - p + 1, 0), np.minimum(i + f, n - 1)
            with np.errstate(over="ignore"):
                s = cs[hi + 1] - cs[lo]
            cnt = cc[hi + 1] - cc[lo]
        for kern in kerns:
            got, gv = run_gpu(gx, col, p, f, 3, "sum", kern)
            assert np.array_equal(gv, cnt >= 3) and np.array_equal(got[gv], s[gv])
            got, gv = run_gpu(gx, col, p, f, 0, "count_valid", kern)
            assert gv.all() and np.array_equal(got, cnt.astype(np.int32))


# ------------------------------------------------------------------------------------------------ DataFrame.rolling against pandas
@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("window", [1, 3, 4])
def test_dataframe_rolling_against_pandas(gx, TS, window, center):
    import pandas as pd
    from cudf_amd import DataFrame
    T, _ = TS
    n = T + 37
    rng = np.random.default_rng(61)
    pdf = pd.DataFrame({"i": rng.integers(-1000, 1000, n).astype(np.int64), "f": (rng.random(n) - 0.5) * 100,
                        "g": ((rng.random(n) - 0.5) * 100).astype(np.float32)})
    df = DataFrame.from_pandas(pdf)
    for mp in sorted({1, window}) + [None]:
        want_roll = pdf.rolling(window, min_periods=mp, center=center)
        got_roll = df.rolling(window, min_periods=mp, center=center)
        for op in ("sum", "min", "max", "mean"):
            want = getattr(want_roll, op)()
            got = getattr(got_roll, op)()
            for name in pdf.columns:
                c = got[name]
                v = c.valid_numpy()
                v = np.ones(n, bool) if v is None else v
                w = want[name].to_numpy()
                assert np.array_equal(v, ~np.isnan(w)), (window, center, mp, op, name)       # where pandas has NaN the result is null
                g = c.to_numpy().astype(np.float64)[v]
                if name == "i" and op != "mean":
                    assert np.array_equal(g, w[v])
                else:
                    # pandas' own sums are streaming (add / remove): the comparison is against the exact window result
                    f = (window - 1) // 2 if center else 0
                    ref = reference(pdf[name].to_numpy(), None, window - f, f)
                    check(ref, pdf[name].dtype, op, window if mp is None else mp, c.to_numpy(), v, (window, center, mp, op, name))
                    assert np.allclose(g, w[v], rtol=1e-4, atol=1e-3)                       # and pandas agrees to its own accuracy


# ------------------------------------------------------------------------------------------------ the C++ surface
def test_cpp_rolling_tests_binary(gx):
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "cudf_rolling_tests")], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "15 run, 0 failed" in r.stdout
