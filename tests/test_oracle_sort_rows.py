"""Pins the comparator reference of multi-column sorts (oracle.cudf_oracle.sorted_order_rows / is_sorted_rows) on the CPU.

The reference orders the rows of a table with the lexicographic row comparator (cpp/src/sort/sort_impl.cuh:61-93): per column nulls
equivalent and placed by null_order (flipped for DESCENDING), NaN equivalent and greater than every number, -0.0 == +0.0
(row_operator/common_utils.cuh:157-169); rows equal on the whole tuple keep their row order.  The single-column radix rule (a
DESCENDING NaN block in REVERSE row order, sorted_order_radix.cu:37-48) is not part of it.  Checked here against a brute-force
comparator written from those rules alone, against orc.sorted_order_table where there are no nulls, and against the single-column
oracle where they must agree.  The generators below also feed tests/test_gpu_sort_float_ties.py."""
import functools
import math

import numpy as np
import pytest

from oracle import cudf_oracle as orc

NAN_BITS = {np.dtype("float64"): [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000077, 0xFFF0000000000001, 0x7FF00000DEADBEEF],
            np.dtype("float32"): [0x7FC00000, 0xFFC00000, 0x7FC00077, 0xFF800001, 0x7F80BEEF]}


def float_key(rng, n, dtype, p_nan=0.05):
    """a float key with ~p_nan NaN of both signs and 5 payloads, -0.0 and +0.0 in the same ties, +-inf, denormals and a small
    domain of ordinary values, so that ties are common"""
    dt = np.dtype(dtype)
    u = np.dtype(f"u{dt.itemsize}")
    f = (rng.integers(-8, 8, n) * 0.5).astype(dt)
    r = rng.random(n)
    f[(r >= 0.05) & (r < 0.10)] = dt.type(0.0)
    f[(r >= 0.10) & (r < 0.15)] = dt.type(-0.0)
    f[(r >= 0.15) & (r < 0.17)] = dt.type(np.inf)
    f[(r >= 0.17) & (r < 0.19)] = dt.type(-np.inf)
    tiny = np.finfo(dt).smallest_subnormal
    den = (r >= 0.19) & (r < 0.22)
    f[den] = (rng.integers(-3, 4, int(den.sum())) * tiny).astype(dt)
    nan = r < p_nan
    f.view(u)[nan] = np.array(NAN_BITS[dt], u)[rng.integers(0, len(NAN_BITS[dt]), int(nan.sum()))]
    return f


def int_key(rng, n, dtype=np.int32, domain=5):
    return rng.integers(-domain // 2, domain - domain // 2, n).astype(dtype)


def lsd_model(cols, valids=None, ascending=True, null_before=True):
    """the per-column composition the tree used to run below 2^18 rows: LSD over the columns, each pass the single-column
    oracle (radix NaN rule included) -- the model of the bug the comparator reference replaces"""
    k = len(cols)
    valids = orc._per_column(valids, k, None)
    asc = orc._per_column(ascending, k, True)
    nb = orc._per_column(null_before, k, True)
    n = len(cols[0])
    order = np.arange(n)
    for c in range(k - 1, -1, -1):
        ok = None if valids[c] is None else np.asarray(valids[c], bool)[order]
        order = order[orc.sorted_order(np.asarray(cols[c])[order], ok, asc[c], nb[c])]
    return order.astype(np.int32)


def brute_order(cols, valids, ascending, null_before):
    """the comparator written out element by element (functools.cmp_to_key), with the row as the last tie-break"""
    k = len(cols)
    n = len(cols[0])

    def cmp_values(x, y):
        x, y = float(x), float(y)
        if math.isnan(x) or math.isnan(y):
            return (math.isnan(x) > math.isnan(y)) - (math.isnan(x) < math.isnan(y))   # NaN == NaN, NaN > every number
        return (x > y) - (x < y)                                                          # -0.0 == +0.0

    def cmp_rows(i, j):
        for c in range(k):
            vi = True if valids[c] is None else bool(valids[c][i])
            vj = True if valids[c] is None else bool(valids[c][j])
            if not vi or not vj:
                if vi == vj:
                    continue
                nulls_first = null_before[c] != (not ascending[c])
                return (-1 if not vi else 1) * (1 if nulls_first else -1)
            r = cmp_values(cols[c][i], cols[c][j])
            if r:
                return r if ascending[c] else -r
        return (i > j) - (i < j)

    return np.array(sorted(range(n), key=functools.cmp_to_key(cmp_rows)), np.int32)


def _small_table(rng):
    n = int(rng.integers(0, 40))
    fdt = [np.float32, np.float64][int(rng.integers(0, 2))]
    cols = [float_key(rng, n, fdt, p_nan=0.3), int_key(rng, n, np.int32, 3)]
    if rng.random() < 0.5:
        cols = cols[::-1]
    if rng.random() < 0.4:
        cols.append(float_key(rng, n, [np.float64, np.float32][int(rng.integers(0, 2))], p_nan=0.3))
    valids = [(rng.random(n) >= 0.2) if rng.random() < 0.6 else None for _ in cols]
    return cols, valids


@pytest.mark.parametrize("seed", range(8))
def test_rows_match_brute_force_comparator(seed):
    """(a) 8 x 40 small random tables (float32 / float64 with NaN of both signs and several payloads, +-0.0, +-inf, denormals,
    nulls, a small-domain int column), every direction and null-precedence combination of the first two columns"""
    rng = np.random.default_rng(1000 + seed)
    for _ in range(40):
        cols, valids = _small_table(rng)
        k = len(cols)
        for a0 in (True, False):
            for a1 in (True, False):
                for b0 in (True, False):
                    for b1 in (True, False):
                        asc = [a0, a1] + [bool(rng.integers(0, 2)) for _ in range(k - 2)]
                        nb = [b0, b1] + [bool(rng.integers(0, 2)) for _ in range(k - 2)]
                        want = brute_order(cols, valids, asc, nb)
                        got = orc.sorted_order_rows(cols, valids, asc, nb)
                        np.testing.assert_array_equal(got, want, err_msg=f"{[c.tolist() for c in cols]} {valids} {asc} {nb}")
                        assert orc.is_sorted_rows([c[got] for c in cols], [None if v is None else v[got] for v in valids], asc, nb)


def test_rows_equal_table_oracle_without_nulls():
    """(b) no nulls: sorted_order_rows is orc.sorted_order_table, 200 tables x 4 direction pairs, sizes up to 3000"""
    rng = np.random.default_rng(7)
    for t in range(200):
        n = int(rng.integers(1, 3000))
        cols = [float_key(rng, n, [np.float32, np.float64][t % 2], p_nan=0.1), int_key(rng, n, np.int64, 7)]
        if t % 3 == 0:
            cols = cols[::-1]
        for asc in ([True, True], [True, False], [False, True], [False, False]):
            np.testing.assert_array_equal(orc.sorted_order_rows(cols, None, asc), orc.sorted_order_table(cols, asc))
            np.testing.assert_array_equal(orc.sorted_order_rows(cols, [None, None], asc, [False, False]),
                                          orc.sorted_order_table(cols, asc))


def test_single_nullable_float_column_equals_single_column_oracle():
    """one float column WITH nulls takes the reference's comparator path (sort_column_impl.cuh:35-57), which orc.sorted_order already
    restates: the two references agree in every direction x precedence combination"""
    rng = np.random.default_rng(3)
    for dt in (np.float32, np.float64):
        f = float_key(rng, 5000, dt, p_nan=0.1)
        valid = rng.random(5000) >= 0.1
        for asc in (True, False):
            for nb in (True, False):
                np.testing.assert_array_equal(orc.sorted_order_rows([f], [valid], asc, nb), orc.sorted_order(f, valid, asc, nb))


def test_issue_example_and_lsd_model_differs():
    """f = [nan, 1, nan, 2, nan] DESCENDING, b = [1, 5, 2, 6, 3] ASCENDING: the NaN rows tie on f and fall to b (row order here)"""
    f = np.array([np.nan, 1, np.nan, 2, np.nan])
    b = np.array([1, 5, 2, 6, 3], np.int32)
    assert orc.sorted_order_rows([f, b], None, [False, True]).tolist() == [0, 2, 4, 3, 1]
    assert lsd_model([f, b], None, [False, True]).tolist() == [4, 2, 0, 3, 1]
    assert brute_order([f, b], [None, None], [False, True], [True, True]).tolist() == [0, 2, 4, 3, 1]
    # the literal of cudf::is_sorted DESCENDING with two NaN in front of a number
    assert orc.is_sorted_rows([np.array([np.nan, np.nan, 1.0])], None, False)
    assert not orc.is_sorted_rows([np.array([np.nan, 1.0, np.nan])], None, False)
    assert orc.is_sorted_rows([np.array([-0.0, 0.0, -0.0, 1.0])], None, True)


def test_segmented_rewrite_keeps_integer_expectations():
    """segmented_sorted_order is sorted_order_rows over (segment id, keys...); on integer keys with nulls -- the inputs of
    test_gpu_cpp_parity's segmented case, smaller -- it equals the per-column composition with a final stable sort on the id"""
    rng = np.random.default_rng(11)
    n = 20_000
    cuts = np.sort(rng.choice(np.arange(100, n - 100), 400, replace=False))
    cuts = np.sort(np.concatenate([cuts[:5], cuts[5:6].repeat(3), cuts[6:], [n - 77]])).astype(np.int32)
    cols = [rng.integers(0, 50, n).astype(np.int32), rng.integers(-10**9, 10**9, n).astype(np.int64)]
    valids = [rng.random(n) >= 0.1, None]
    ids = np.arange(n, dtype=np.int64)
    for j in range(len(cuts) - 1):
        ids[cuts[j]:cuts[j + 1]] = cuts[j + 1]
    ids[: cuts[0]] = np.arange(cuts[0])
    ids[cuts[-1]:] = np.arange(cuts[-1], n) + 1
    for asc, nb in (([True, False], [True, True]), ([False, True], [False, True])):
        order = lsd_model(cols, valids, asc, nb).astype(np.int64)
        want = order[np.argsort(ids[order], kind="stable")]
        np.testing.assert_array_equal(orc.segmented_sorted_order(cols, cuts, valids, asc, nb), want)


def test_generators_plant_the_ties():
    """the float generator holds what the GPU cases rely on: NaN of both signs and >= 3 payloads, both zeros, infinities, denormals"""
    rng = np.random.default_rng(5)
    for dt in (np.float32, np.float64):
        f = float_key(rng, 100_003, dt)
        u = f.view(f"u{f.dtype.itemsize}")
        nan = np.isnan(f)
        assert 0.03 < nan.mean() < 0.07
        assert len(np.unique(u[nan])) >= 3 and np.signbit(f[nan]).any() and (~np.signbit(f[nan])).any()
        assert (u == 0).any() and (f == 0).sum() > (u == 0).sum()        # +0.0 and -0.0
        assert np.isposinf(f).any() and np.isneginf(f).any()
        assert ((f != 0) & (np.abs(f) < np.finfo(dt).tiny)).any()
