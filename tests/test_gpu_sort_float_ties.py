"""GPU: the tie order of NaN rows in DESCENDING float keys on every multi-column sort path, pinned bit-exact to the comparator
reference (orc.sorted_order_rows).

The reference orders a table's rows with the lexicographic row comparator (cpp/src/sort/sort_impl.cuh:61-93): tied NaNs are equal, so
their order falls to the later keys and then to the row.  Only an order of ONE column keeps the radix path's rule that puts a
DESCENDING NaN block in reverse row order (sorted_order_radix.cu:37-48; orc.sorted_order).  The C++ layer sorts a table with the
per-column loop below TABLE_PATH_MIN_ROWS = 2^18 rows or when a key column has nulls (cudf_amd/cpp/src/sorting.cpp), and with one word
sort on the tuple (gx_sorted_order_table) otherwise; DataFrame.sort_values has the same split (_TABLE_PATH_MIN_ROWS).  The cases pin
the path by construction: n in {1, 2, 3, 65, 4097, 2^18 - 1} -> the loop, n = 2^18 + 3 without nulls -> the table path, n = 2^18 + 3
with a nullable int key -> the loop again, a nullable float key -> the validity split.

Every DESCENDING case with a non-nullable float key from 65 rows up asserts on the CPU that its float key holds a tie of >= 2 NaN rows
that differ in a later key and that the model of the per-column composition with the single-column rule (lsd_model) differs from
the comparator order, so that no case silently stops testing the tie order.  Nullable float keys are exempt: the validity split
already follows the comparator, and the model agrees with it there.  Float outputs are compared as bytes (NaN payloads, -0.0)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cudf_oracle as orc
from tests.test_gpu_cpp_parity import Dev, Out, _ulp_ok, shim  # noqa: F401  (fixture)
from tests.test_oracle_sort_rows import NAN_BITS, float_key, int_key, lsd_model

TABLE_PATH_MIN_ROWS = 1 << 18          # cudf_amd/cpp/src/sorting.cpp, cudf_amd/dataframe.py _TABLE_PATH_MIN_ROWS
LSD_SIZES = [1, 2, 3, 65, 4097, TABLE_PATH_MIN_ROWS - 1]
BIG = TABLE_PATH_MIN_ROWS + 3
DIRS = [(True, True), (True, False), (False, True), (False, False)]
FDT = {1: np.float64, 2: np.float32, 3: np.float64, 65: np.float32, 4097: np.float64, TABLE_PATH_MIN_ROWS - 1: np.float32,
       BIG: np.float64}


def _nan(dt, which):
    u = np.dtype(f"u{np.dtype(dt).itemsize}")
    return np.array([NAN_BITS[np.dtype(dt)][which]], u).view(dt)[0]


def _plant(f, later, i, j):
    """rows i < j: NaN (different payloads, both signs) in the float key, different values in the later key"""
    f[i], f[j] = _nan(f.dtype, 1), _nan(f.dtype, 2)
    later[i], later[j] = 2, -2


def _table(n, seed, fdt=None, *, null_int=False, null_float=False, third=False):
    """[f, b (, c)]: a float key with ~5 % NaN, a small-domain int key, a wide int64 third key; valids per column or None"""
    rng = np.random.default_rng(seed)
    fdt = fdt or FDT[n]
    f, b = float_key(rng, n, fdt), int_key(rng, n, np.int32, 5)
    cols = [f, b] + ([rng.integers(-2**40, 2**40, n, dtype=np.int64)] if third else [])
    valids = [None] * len(cols)
    if null_int:
        valids[1] = rng.random(n) >= 0.1
    if null_float:
        valids[0] = rng.random(n) >= 0.1
    if n >= 65:
        i = int(rng.integers(0, n // 2))
        j = int(rng.integers(i + 1, n))
        _plant(f, b, i, j)
        for v in valids:
            if v is not None:
                v[[i, j]] = True
    return cols, valids


def _guard(cols, valids, asc, nb, fi=0):
    """the DESCENDING float key cols[fi] (no nulls) holds a NaN tie of >= 2 rows that differ in the next key, and the per-column model
    with the single-column NaN rule orders the table differently from the comparator"""
    n = len(cols[0])
    if n < 65 or asc[fi] or valids[fi] is not None:
        return
    rows = np.flatnonzero(np.isnan(cols[fi]))
    pre = _row_keys(cols[:fi], valids[:fi])[rows] if fi else np.zeros((len(rows), 1), np.uint64)   # the keys before the float key
    later = _row_keys(cols[fi + 1:fi + 2], valids[fi + 1:fi + 2])[rows]
    pairs = np.unique(np.concatenate([pre, later], 1), axis=0)
    assert len(pairs) and np.unique(pairs[:, :pre.shape[1]], axis=0, return_counts=True)[1].max() >= 2, \
        "no NaN tie that differs in a later key"
    assert not np.array_equal(lsd_model(cols, valids, asc, nb), orc.sorted_order_rows(cols, valids, asc, nb)), \
        "the per-column model agrees with the comparator: the case no longer tests the tie order"


def _same_bytes(got, want, msg=""):
    """bit-exact equality (NaN payloads, -0.0), reported as the differing positions of the bit images -- an assert on two .tobytes()
    of a few MB makes pytest diff them byte by byte for minutes"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    u = np.dtype(f"u{got.dtype.itemsize}")
    np.testing.assert_array_equal(got.view(u), want.view(u), err_msg=msg)


def _args(devs, asc=None, nb=None):
    k = len(devs)
    dt = (ctypes.c_int * k)(*[d.tid for d in devs])
    dp = (ctypes.c_void_p * k)(*[d.p.value for d in devs])
    vp = (ctypes.c_void_p * k)(*[(d.mp.value if d.mp is not None else None) for d in devs])
    nl = (ctypes.c_int * k)(*[d.nulls for d in devs])
    de = (ctypes.c_int * k)(*[0 if a else 1 for a in (asc or [True] * k)])
    nbv = (ctypes.c_int * k)(*[1 if b else 0 for b in (nb or [True] * k)])
    return dt, dp, vp, nl, de, nbv


def _sorted_order(shim, cols, valids, asc, nb, stable):
    n = len(cols[0])
    devs = [Dev(c, v) for c, v in zip(cols, valids)]
    dt, dp, vp, nl, de, nbv = _args(devs, asc, nb)
    out = Out(np.int32, n)
    shim("shim_table_sorted_order", len(cols), dt, dp, vp, nl, n, de, nbv, stable, out.p)
    return out.get(n)


def _is_sorted(shim, cols, valids, asc, nb=None):
    n = len(cols[0])
    devs = [Dev(c, v) for c, v in zip(cols, valids)]
    dt, dp, vp, nl, de, nbv = _args(devs, asc, nb)
    res = ctypes.c_int(-1)
    shim("shim_is_sorted", len(cols), dt, dp, vp, nl, n, de, nbv, ctypes.byref(res))
    assert res.value in (0, 1)
    return bool(res.value)


def _precs(valids):
    return [(True, True), (False, False), (True, False), (False, True)] if any(v is not None for v in valids) else [(True, True)]


def _check_orders(shim, cols, valids, fi=0, dirs=DIRS):
    for asc2 in dirs:
        asc = list(asc2) + [True] * (len(cols) - 2)
        for nb2 in _precs(valids):
            nb = list(nb2) + [True] * (len(cols) - 2)
            _guard(cols, valids, asc, nb, fi)
            want = orc.sorted_order_rows(cols, valids, asc, nb)
            for stable in (0, 1):
                got = _sorted_order(shim, cols, valids, asc, nb, stable)
                np.testing.assert_array_equal(got, want, err_msg=f"asc={asc} null_before={nb} stable={stable}")


# ---------------------------------------------------------------------------------------------------------------------
# sorted_order / stable_sorted_order of a table
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", LSD_SIZES)
def test_sorted_order_loop(shim, n):
    """below 2^18 rows, no nulls: the per-column loop, all four direction pairs"""
    cols, valids = _table(n, 100 + n)
    _check_orders(shim, cols, valids)


@pytest.mark.parametrize("n", [65, 4097, TABLE_PATH_MIN_ROWS - 1])
def test_sorted_order_loop_float_in_the_middle(shim, n):
    """[b, f, c]: the NaN tie sits inside ties of the leading int key and falls to the third key"""
    rng = np.random.default_rng(n)
    f, b = float_key(rng, n, FDT[n]), int_key(rng, n, np.int32, 3)
    c = rng.integers(-2**40, 2**40, n, dtype=np.int64)
    i, j = int(rng.integers(0, n // 2)), int(rng.integers(n // 2, n))
    b[j] = b[i]
    _plant(f, c, i, j)
    cols = [b, f, c]
    for asc in ([True, False, True], [False, False, False], [True, True, False]):
        _guard(cols, [None] * 3, asc, [True] * 3, fi=1)
        want = orc.sorted_order_rows(cols, None, asc)
        for stable in (0, 1):
            np.testing.assert_array_equal(_sorted_order(shim, cols, [None] * 3, asc, [True] * 3, stable), want)


def test_sorted_order_table_path(shim):
    """2^18 + 3 rows without nulls: one word sort on the tuple"""
    cols, valids = _table(BIG, 7)
    _check_orders(shim, cols, valids)
    cols, valids = _table(BIG, 8, np.float32, third=True)
    _check_orders(shim, cols, valids)


def test_sorted_order_nullable_int_key_at_scale(shim):
    """2^18 + 3 rows, the int key nullable: the per-column loop again, both null precedences"""
    cols, valids = _table(BIG, 9, null_int=True)
    _check_orders(shim, cols, valids)


@pytest.mark.parametrize("n", [3, 4097, BIG])
def test_sorted_order_nullable_float_key(shim, n):
    """the float key nullable: its pass is the validity split, which orders the valid rows under the comparator"""
    cols, valids = _table(n, 11 + n, null_float=True)
    _check_orders(shim, cols, valids)


# ---------------------------------------------------------------------------------------------------------------------
# sort / stable_sort / sort_by_key / stable_sort_by_key
# ---------------------------------------------------------------------------------------------------------------------
def _check_gathered(outs, out_valids, cols, valids, order):
    for o, ov, c, v in zip(outs, out_valids, cols, valids):
        n = len(c)
        got, want = o.get(n), c[order]
        wv = np.ones(n, bool) if v is None else v[order]
        np.testing.assert_array_equal(ov.valid(n), wv)
        _same_bytes(got[wv], want[wv])


@pytest.mark.parametrize("n,nulls", [(1, ""), (2, ""), (65, ""), (4097, ""), (TABLE_PATH_MIN_ROWS - 1, ""), (BIG, ""),
                                     (BIG, "int"), (4097, "float")])
def test_sort_and_sort_by_key(shim, n, nulls):
    cols, valids = _table(n, 200 + n, null_int=nulls == "int", null_float=nulls == "float")
    k = len(cols)
    rng = np.random.default_rng(n)
    vals = [np.arange(n, dtype=np.int32), float_key(rng, n, np.float64)]
    vvalids = [None, rng.random(n) >= 0.2]
    kdevs = [Dev(c, v) for c, v in zip(cols, valids)]
    vdevs = [Dev(c, v) for c, v in zip(vals, vvalids)]
    for asc in DIRS:
        for nb in _precs(valids):
            _guard(cols, valids, asc, nb)
            order = orc.sorted_order_rows(cols, valids, list(asc), list(nb))
            dt, dp, vp, nl, de, nbv = _args(kdevs, list(asc), list(nb))
            vdt, vdp, vvp, vnl, _, _ = _args(vdevs)
            for stable in (0, 1):
                outs = [Out(c.dtype, n, mask=True) for c in cols]
                shim("shim_sort", k, dt, dp, vp, nl, n, de, nbv, stable, (ctypes.c_void_p * k)(*[o.p.value for o in outs]),
                     (ctypes.c_void_p * k)(*[o.mp.value for o in outs]), None)
                _check_gathered(outs, outs, cols, valids, order)
                vouts = [Out(c.dtype, n, mask=True) for c in vals]
                shim("shim_sort_by_key", 2, vdt, vdp, vvp, vnl, k, dt, dp, vp, nl, n, de, nbv, stable,
                     (ctypes.c_void_p * 2)(*[o.p.value for o in vouts]), (ctypes.c_void_p * 2)(*[o.mp.value for o in vouts]), None)
                _check_gathered(vouts, vouts, vals, vvalids, order)


# ---------------------------------------------------------------------------------------------------------------------
# segmented_sorted_order / stable_segmented_sorted_order
# ---------------------------------------------------------------------------------------------------------------------
def _cuts(n):
    """segments of sizes 0, 1, 2 and two long ones, with rows before the first and after the last offset outside every segment"""
    h = max(1, n // 20)
    cuts = [h, h, h + 1, h + 3, h + 3 + (n - 2 * h - 3) // 2, n - h]
    return np.array(cuts, np.int32)


def _segment_ids(cuts, n):
    ids = np.arange(n, dtype=np.int64)
    for j in range(len(cuts) - 1):
        ids[cuts[j]:cuts[j + 1]] = cuts[j + 1]
    ids[: cuts[0]] = np.arange(cuts[0])
    ids[cuts[-1]:] = np.arange(cuts[-1], n) + 1
    return ids


@pytest.mark.parametrize("n", [65, 4097, TABLE_PATH_MIN_ROWS - 1, BIG])
def test_segmented_sorted_order(shim, n):
    import torch
    cols, valids = _table(n, 300 + n)
    cuts = _cuts(n)
    rng = np.random.default_rng(n)
    lo, hi = int(cuts[3]), int(cuts[4])
    i = int(rng.integers(lo, (lo + hi) // 2))
    _plant(cols[0], cols[1], i, int(rng.integers(i + 1, hi)))      # a NaN tie inside one long segment
    ids = _segment_ids(cuts, n)
    devs = [Dev(c, v) for c, v in zip(cols, valids)]
    off = torch.from_numpy(cuts.copy()).cuda()
    for asc in DIRS:
        _guard([ids] + cols, [None] + valids, [True] + list(asc), [True] * 3, fi=1)
        want = orc.segmented_sorted_order(cols, cuts, valids, list(asc), [True, True])
        np.testing.assert_array_equal(want, orc.sorted_order_rows([ids] + cols, None, [True] + list(asc)))
        dt, dp, vp, nl, de, nbv = _args(devs, list(asc))
        for stable in (0, 1):
            out = Out(np.int32, n)
            shim("shim_segmented_sorted_order", 2, dt, dp, vp, nl, n, ctypes.c_void_p(off.data_ptr()), len(cuts), de, nbv, stable,
                 out.p)
            np.testing.assert_array_equal(out.get(n), want, err_msg=f"asc={asc} stable={stable}")


# ---------------------------------------------------------------------------------------------------------------------
# is_sorted
# ---------------------------------------------------------------------------------------------------------------------
def _row_keys(cols, valids):
    """per row the columns' (validity, sortable bits) pairs: equal keys <=> rows equal under the comparator"""
    keys = []
    for c, v in zip(cols, valids):
        bits = orc.sortable_bits(c).astype(np.uint64)
        ok = np.ones(len(c), bool) if v is None else np.asarray(v, bool)
        keys += [ok.astype(np.uint64), np.where(ok, bits, 0)]
    return np.stack(keys, 1)


def _swapped(cols, valids, p):
    cs = [c.copy() for c in cols]
    vs = [None if v is None else v.copy() for v in valids]
    for x in cs + [v for v in vs if v is not None]:
        x[[p, p + 1]] = x[[p + 1, p]]
    return cs, vs


def _swap_positions(cols, valids):
    """adjacent pairs of unequal rows: the first, the last, a NaN / number boundary of the float key cols[0], and (where there is one)
    a pair inside a NaN tie of the float key that differs in the next key"""
    k = _row_keys(cols, valids)
    uneq = np.flatnonzero(np.any(k[1:] != k[:-1], axis=1))
    if len(uneq) == 0:
        return {}
    pos = {"first": int(uneq[0]), "last": int(uneq[-1])}
    f = cols[0]
    fv = np.ones(len(f), bool) if valids[0] is None else valids[0]
    isn = np.isnan(f) & fv
    num = ~np.isnan(f) & fv
    b = np.flatnonzero((isn[:-1] & num[1:]) | (num[:-1] & isn[1:]))
    if len(b):
        pos["nan_boundary"] = int(b[0])
    if len(cols) > 1:
        t = np.flatnonzero(isn[:-1] & isn[1:] & np.any(k[1:, 2:4] != k[:-1, 2:4], axis=1))
        if len(t):
            pos["nan_tie"] = int(t[len(t) // 2])
    return pos


@pytest.mark.parametrize("n", [65, 4097, BIG])
def test_is_sorted_true_and_false_after_one_swap(shim, n):
    """True for tables gathered through the comparator order (one float column with and without nulls, float x int; both directions),
    False after one adjacent swap of two rows that are unequal under the comparator"""
    cols, valids = _table(n, 400 + n)
    ncols, nvalids = _table(n, 500 + n, null_float=True)
    tables = [("float", [cols[0]], [None]), ("float_nulls", [ncols[0]], [nvalids[0]]), ("float_int", cols, valids)]
    for name, tc, tv in tables:
        for asc1 in (True, False):
            asc = [asc1] + [True] * (len(tc) - 1)
            for nb1 in ((True, False) if tv[0] is not None else (True,)):
                nb = [nb1] * len(tc)
                order = orc.sorted_order_rows(tc, tv, asc, nb)
                sc = [c[order] for c in tc]
                sv = [None if v is None else v[order] for v in tv]
                assert orc.is_sorted_rows(sc, sv, asc, nb)
                assert _is_sorted(shim, sc, sv, asc, nb), (name, asc, nb)
                pos = _swap_positions(sc, sv)
                assert {"first", "last", "nan_boundary"} <= set(pos), (name, pos)
                if name == "float_int":
                    assert "nan_tie" in pos, pos
                for where, p in pos.items():
                    wc, wv = _swapped(sc, sv, p)
                    assert not orc.is_sorted_rows(wc, wv, asc, nb)
                    assert not _is_sorted(shim, wc, wv, asc, nb), (name, asc, nb, where, p)


def test_is_sorted_literals(shim):
    """{NaN, NaN, 1.0} DESCENDING is in order (the comparator: NaN greatest, NaNs equal); a NaN behind a number is not"""
    for dt in (np.float32, np.float64):
        for vals, asc, want in (([np.nan, np.nan, 1.0], False, True), ([_nan(dt, 1), _nan(dt, 2), 1.0], False, True),
                                ([np.nan, 1.0, np.nan], False, False), ([1.0, np.nan, np.nan], True, True),
                                ([-0.0, 0.0, -0.0, 1.0], True, True), ([1.0, -0.0, 0.0, -0.0], False, True),
                                ([1.0, np.nan], False, False)):
            c = np.array(vals, dt)
            assert orc.is_sorted_rows([c], None, asc) == want
            assert _is_sorted(shim, [c], [None], [asc]) == want, (dt, vals, asc)


def test_is_sorted_int_column_at_scale(shim):
    """one int64 column without nulls at 2^18 + 3 rows: the streaming pass, violations at the first, the last and random pairs"""
    rng = np.random.default_rng(21)
    v = np.sort(rng.integers(-1000, 1000, BIG).astype(np.int64))
    for asc in (True, False):
        s = v if asc else v[::-1].copy()
        assert _is_sorted(shim, [s], [None], [asc])
        uneq = np.flatnonzero(s[1:] != s[:-1])
        for p in [int(uneq[0]), int(uneq[-1])] + [int(x) for x in rng.choice(uneq, 3, replace=False)]:
            w = s.copy()
            w[[p, p + 1]] = w[[p + 1, p]]
            assert not _is_sorted(shim, [w], [None], [asc]), (asc, p)
        t = np.flatnonzero(s[1:] == s[:-1])[0]     # swapping equal rows keeps the column in order
        w = s.copy()
        w[[t, t + 1]] = w[[t + 1, t]]
        assert _is_sorted(shim, [w], [None], [asc])


# ---------------------------------------------------------------------------------------------------------------------
# DataFrame.sort_values with two keys
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,null_int", [(65, False), (4097, False), (TABLE_PATH_MIN_ROWS - 1, False), (BIG, False), (BIG, True)])
def test_dataframe_two_keys_float_descending(n, null_int):
    """the row order equals the comparator's (pandas places NaN by na_position, so it is not the reference here); which path ran is
    read off the calls of ops.sorted_order_table: the table path sorts the 2-column tuple in one call, the loop never does"""
    import cudf_amd
    from cudf_amd import Column
    from cudf_amd import dataframe as dfm
    assert dfm._TABLE_PATH_MIN_ROWS == TABLE_PATH_MIN_ROWS
    cols, valids = _table(n, 600 + n, null_int=null_int)
    f, b = cols
    calls = []
    orig = cudf_amd.ops.sorted_order_table
    cudf_amd.ops.sorted_order_table = lambda cs, asc=True: (calls.append(len(cs)), orig(cs, asc))[1]
    try:
        for asc in ([False, True], [False, False]):
            for na in ("last", "first"):
                calls.clear()
                df = cudf_amd.DataFrame({"f": f, "b": Column.from_numpy(b, valids[1]) if null_int else b,
                                         "row": np.arange(n, dtype=np.int32)})
                nb = [a ^ (na == "last") for a in asc]
                _guard(cols, valids, asc, nb)
                got = df.sort_values(["f", "b"], ascending=asc, na_position=na)
                want = orc.sorted_order_rows(cols, valids, asc, nb)
                np.testing.assert_array_equal(got["row"].to_numpy(), want)
                _same_bytes(got["f"].to_numpy(), f[want])
                table_path = n >= TABLE_PATH_MIN_ROWS and not null_int
                assert (2 in calls) == table_path, calls
                if not table_path:
                    assert all(c == 1 for c in calls), calls
    finally:
        cudf_amd.ops.sorted_order_table = orig


# ---------------------------------------------------------------------------------------------------------------------
# single-column orders keep the radix rule
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float32, np.float64])
def test_single_column_keeps_radix_rule(shim, dt):
    """one float column DESCENDING (NaN / +-0 ties): sorted_order, rank (five methods) and top_k equal the single-column oracle"""
    for n in (65, 4097, BIG):
        rng = np.random.default_rng(n)
        f = float_key(rng, n, dt)
        assert np.isnan(f).sum() >= 2
        want = orc.sorted_order(f, None, False)
        np.testing.assert_array_equal(_sorted_order(shim, [f], [None], [False], [True], 1), want)
        d = Dev(f)
        for method in (orc.RANK_FIRST, orc.RANK_AVERAGE, orc.RANK_MIN, orc.RANK_MAX, orc.RANK_DENSE):
            for percentage in (False, True):
                as_f64 = percentage or method == orc.RANK_AVERAGE
                out = Out(np.float64 if as_f64 else np.int32, n, mask=True)
                nulls = ctypes.c_int(-1)
                shim("shim_rank", d.tid, d.p, None, n, 0, method, 1, 0, 1, 1 if percentage else 0, out.p, out.mp, ctypes.byref(nulls))
                wr, _ = orc.rank(f, None, method, False, False, True, percentage)
                got = out.get(n)
                if as_f64:
                    assert _ulp_ok(got, wr, 1), (n, method, percentage)
                else:
                    np.testing.assert_array_equal(got, wr)
        for k in (1, int(np.isnan(f).sum()) // 2 + 1, n // 3, n - 1):
            ov, oi = Out(f.dtype, n), Out(np.int32, n)
            cnt = ctypes.c_int(-1)
            shim("shim_top_k", d.tid, d.p, None, n, 0, k, 1, ov.p, oi.p, ctypes.byref(cnt))
            wv, wi, _ = orc.top_k(f, k, True)
            assert cnt.value == len(wv)
            np.testing.assert_array_equal(oi.get(cnt.value), wi)
            _same_bytes(ov.get(cnt.value), wv)
