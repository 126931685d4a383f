"""GPU: float SUM where a compensated sum can differ from the reference's plain addition, and where it must beat it.

Every float SUM of the package is compensated with two_sum (DDSum in gx_reduce_scan.hip; comp_add in
gx_groupby.hip).  The error term of an addition that meets +-inf or overflows is inf - inf = NaN; the first part of this file
pins that no such NaN reaches a result: a sum or prefix is +-inf / NaN exactly where plain addition gives it
(oracle exact_sum / exact_prefix_sums), and everything finite stays within 1 ulp of the exact value.  The second part feeds
sums whose terms are ~1e7 times larger than the result, where an uncompensated double accumulator is thousands of ulps off
(asserted on the same input), so a compensation term dropped at a wave, chunk, partition or merge boundary shows.

Tolerance (all of this file): 1 ulp of the OUTPUT type against the exact sum rounded to that type -- the double-double error
bound n * 2^-104 * sum|x| is below one ulp of the result while sum|x| / |sum x| < 2^50 / n, and a float32 output rounds the
double result a second time.  The one exception is groupby_scan, which accumulates in plain double (the control of the
non-finite cases): its bound is the textbook m * 2^-53 * sum|x| of a sum of m terms in any order.

GPU time (MI355X): the 177 cases of this file take 6 s together, 1.6 s of it the first import.  Per case: reduce SUM / MEAN
0.01 - 0.3 s (the first call loads the shim), scan 0.01 - 0.2 s, groupby_scan control <= 0.05 s, sort-path groupby 0.01 - 0.03 s,
pinned hash paths 0.01 s, auto path at 600 000 rows 0.1 s, two key columns 0.1 s, DataFrame against pandas 0.7 s,
ill-conditioned reduce + scan 0.07 s, ill-conditioned groupby 0.02 s (their shared CPU reference: 0.2 s per dtype, once).

On the commit before the fix, 99 of the 177 cases fail, each with NaN where the exact sum is +inf or -inf
(profiles/float_sum_nonfinite_vs_parent.txt).
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cudf_oracle as orc
from tests.test_gpu_cpp_parity import Dev, Out, NPT, shim  # noqa: F401  (the shim fixture and the device-column helpers)
from tests.test_gpu_partition_reduce_contract import _reduce_init

KIND = dict(sum=0, mean=10)  # cudf::aggregation::Kind
FLOATS = ["float64", "float32"]
N = 40_003  # ten 4096-row scan chunks, three 16384-row look-back tiles, 157 wavefronts
PLACEMENTS = ["pos_inf", "neg_inf", "pos_then_neg_inf", "nan", "chunk_first_and_column_last", "overflow", "inf_in_null_row"]


@pytest.fixture(scope="module")
def gx():
    import torch
    assert torch.cuda.is_available()
    import cudf_amd  # noqa: F401
    from cudf_amd import Column, ops
    return Column, ops


def _ulps(got, want):
    """distance in units of the last place of the arrays' (common) float type"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.dtype.kind == "f"
    if got.dtype == np.float64:
        return orc.ulp_diff(got, want)
    a, b = got.view(np.int32).astype(np.int64), want.view(np.int32).astype(np.int64)
    a, b = np.where(a < 0, -(2**31) - a, a), np.where(b < 0, -(2**31) - b, b)
    return np.abs(a - b)


def _cast(x, dtype):
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(dtype)


def _check(got, want, what="", slack=None):
    """+-inf / NaN exactly where the exact sum has them (assert_array_equal: NaN == NaN), everything else within 1 ulp.
    slack: absolute error allowed on top of that ulp, per element (0 wherever the 1-ulp bound is proven)."""
    got, want = np.atleast_1d(got), np.atleast_1d(want)
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    nf = ~np.isfinite(want)
    np.testing.assert_array_equal(got[nf], want[nf], err_msg=f"{what}: non-finite results")
    assert np.isfinite(got[~nf]).all(), f"{what}: {int((~np.isfinite(got[~nf])).sum())} results are not finite where the exact sum is"
    d = _ulps(got[~nf], want[~nf])
    if slack is not None:
        w = want[~nf]
        d = np.where(np.abs(got[~nf].astype(np.float64) - w) <= np.spacing(np.abs(w)).astype(np.float64) + slack[~nf], np.minimum(d, 1), d)
    assert d.size == 0 or int(d.max()) <= 1, f"{what}: {int(d.max())} ulps at {int(np.argmax(d))}"


@functools.lru_cache(maxsize=None)
def _column(dtype, placement, nulls):
    """(values, valid or None, exact inclusive prefix sums in float64, number of valid rows): ~40 000 rows of U[-1000, 1000)
    with the non-finite values of `placement` in VALID rows.  Cached: one reference per case, shared by the tests."""
    rng = np.random.default_rng([PLACEMENTS.index(placement), FLOATS.index(dtype), int(nulls)])
    v = (rng.random(N) * 2000 - 1000).astype(dtype)
    valid = (rng.random(N) > 0.2) if (nulls or placement == "inf_in_null_row") else None
    big = 1e308 if dtype == "float64" else 3e38
    pos = {"pos_inf": [12_345], "neg_inf": [23_456], "pos_then_neg_inf": [9_000, 30_000], "nan": [20_001],
           "chunk_first_and_column_last": [16_384, N - 1], "inf_in_null_row": [17_000],
           "overflow": [3, 4_095, 4_096, 10_000, 16_383, 16_384, 30_001, N - 1]}[placement]
    val = {"pos_inf": [np.inf], "neg_inf": [-np.inf], "pos_then_neg_inf": [np.inf, -np.inf], "nan": [np.nan],
           "chunk_first_and_column_last": [np.inf, np.inf], "inf_in_null_row": [np.inf], "overflow": [big] * 8}[placement]
    if placement == "overflow":
        v = np.abs(v) + v.dtype.type(1)  # monotone: every summation order overflows, no prefix comes back
    v[pos] = np.array(val, dtype)
    if valid is not None:
        valid[pos] = placement != "inf_in_null_row"
    x = v.astype(np.float64) if valid is None else np.where(valid, v, 0).astype(np.float64)
    prefix = orc.exact_prefix_sums(x)
    if placement == "inf_in_null_row":
        assert np.isfinite(prefix).all()
    elif placement == "overflow":
        assert np.isfinite(prefix[: pos[1]]).all() and (_cast(prefix[pos[1]:], dtype) == np.inf).all()
    else:
        assert np.isfinite(prefix[: pos[0]]).all() and not np.isfinite(prefix[pos[0]:]).any()
    for a in (v, prefix) + (() if valid is None else (valid,)):
        a.setflags(write=False)
    return v, valid, prefix, N if valid is None else int(valid.sum())


CASES = [pytest.param(d, p, n, id=f"{d}-{p}-{'nulls' if n else 'nonulls'}")
         for d in FLOATS for i, p in enumerate(PLACEMENTS) for n in ([True] if p == "inf_in_null_row" else [False, True])]


# ---------------------------------------------------------------------------------------------------------------------
# cudf::reduce SUM / MEAN, cudf::scan SUM
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,placement,nulls", CASES)
def test_reduce_sum_mean_non_finite(gx, shim, dtype, placement, nulls):  # noqa: F811
    Column, ops = gx
    v, valid, prefix, nvalid = _column(dtype, placement, nulls)
    for out_dtype in (np.float64, np.dtype(dtype).type):
        got, ok = ops.reduce(Column.from_numpy(v, valid), "sum", out_dtype)
        want, wok = orc.reduce(v, "sum", valid, out_dtype)
        assert ok and wok
        np.testing.assert_array_equal(want, _cast(prefix[-1], out_dtype))  # the oracle's entry point and the prefix agree
        _check(np.asarray(got), np.asarray(want), f"reduce sum -> {np.dtype(out_dtype)}")
    got, ok = _reduce_init(shim, v, valid, "mean", np.float64, 0, v.dtype, True, has_init=False)
    want, _ = orc.reduce(v, "mean", valid, np.float64)
    assert ok
    _check(np.asarray(got), np.asarray(want), "reduce mean")


@pytest.mark.parametrize("inclusive", [True, False], ids=["inclusive", "exclusive"])
@pytest.mark.parametrize("dtype,placement,nulls", CASES)
def test_scan_sum_non_finite(gx, dtype, placement, nulls, inclusive):
    Column, ops = gx
    v, valid, prefix, _ = _column(dtype, placement, nulls)
    out = ops.scan(Column.from_numpy(v, valid), "sum", inclusive)
    want = prefix if inclusive else np.concatenate([[0.0], prefix[:-1]])
    ev, em = orc.scan(v, "sum", inclusive, valid, exact=True)
    np.testing.assert_array_equal(ev, _cast(want, dtype))
    sel = np.ones(N, bool) if valid is None else valid
    if valid is not None:
        np.testing.assert_array_equal(out.valid_numpy(), em)
    _check(out.to_numpy()[sel], ev[sel], "scan sum")


# ---------------------------------------------------------------------------------------------------------------------
# groupby::scan SUM: plain double accumulation -- the control (expected to hold before and after the two_sum fix)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,placement,nulls", CASES)
def test_groupby_scan_sum_non_finite_control(gx, dtype, placement, nulls):
    Column, ops = gx
    v, valid, _, _ = _column(dtype, placement, nulls)
    keys = np.sort(np.random.default_rng(1).integers(0, 7, N)).astype(np.int32)
    out = ops.groupby_scan(Column.from_numpy(keys), Column.from_numpy(v, valid), "sum").to_numpy()
    assert out.dtype == v.dtype
    x = v.astype(np.float64) if valid is None else np.where(valid, v, 0).astype(np.float64)
    want, bound = np.empty(N), np.empty(N)
    for g in range(7):
        lo, hi = np.searchsorted(keys, [g, g + 1])
        want[lo:hi] = orc.exact_prefix_sums(x[lo:hi])
        with np.errstate(invalid="ignore", over="ignore"):
            bound[lo:hi] = np.arange(1, hi - lo + 1) * 2.0 ** -53 * np.cumsum(np.abs(x[lo:hi]))  # m terms in double, any order
    want32 = _cast(want, dtype)
    sel = np.ones(N, bool) if valid is None else valid
    nf = ~np.isfinite(want32)
    np.testing.assert_array_equal(out[sel & nf], want32[sel & nf])
    fin = sel & ~nf
    with np.errstate(invalid="ignore"):
        bound = bound + np.abs(want) * (2.0 ** -53 if dtype == "float64" else 2.0 ** -24)  # one rounding to the output type
    assert np.isfinite(out[fin]).all()
    assert np.all(np.abs(out[fin].astype(np.float64) - want[fin]) <= bound[fin])


# ---------------------------------------------------------------------------------------------------------------------
# sort-path groupby SUM / MEAN (gx_segmented_reduce through cudf::groupby::aggregate)
# ---------------------------------------------------------------------------------------------------------------------
def _sort_groupby(shim_call, keys, vals, vvalid, agg):
    n = len(keys)
    dk, dv = Dev(keys), Dev(vals, vvalid)
    ok_, ov = Out(np.int32, n, True), Out(np.float64, n, True)
    kn, vn, g, vt = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    # force_sort = 1: a second NTH_ELEMENT request keeps the request off the hash path
    shim_call("shim_groupby_aggregate", dk.tid, dk.p, dk.mp, dk.nulls, dv.tid, dv.p, dv.mp, dv.nulls, n, KIND[agg], 0, 0, 0, 1,
              ok_.p, ok_.mp, ctypes.byref(kn), ov.p, ov.mp, ctypes.byref(vn), ctypes.byref(g), ctypes.byref(vt))
    G = g.value
    return ok_.get(G), ov.get(G, NPT[vt.value]), ov.valid(G)


def _group_keys(shape, n, rng):
    if shape == "few_long_groups":  # ~n / 7 rows per group: every group spans chunks
        return rng.integers(0, 7, n).astype(np.int32)
    return np.where(rng.random(n) < 0.4, rng.integers(0, 3, n), rng.integers(3, n // 20, n)).astype(np.int32)  # mixed


@pytest.mark.parametrize("shape", ["few_long_groups", "mixed"])
@pytest.mark.parametrize("dtype,placement,nulls", CASES)
def test_sort_path_groupby_sum_mean_non_finite(shim, dtype, placement, nulls, shape):  # noqa: F811
    v, valid, _, _ = _column(dtype, placement, nulls)
    keys = _group_keys(shape, N, np.random.default_rng(2))
    if placement == "overflow":  # the eight large values share a group, so that it overflows whatever the keys drew
        keys = keys.copy()
        keys[[3, 4_095, 4_096, 10_000, 16_383, 16_384, 30_001, N - 1]] = 1
    wk, _, wsum, wok = orc.groupby_sort_agg(keys, v, "sum", None, valid)
    assert placement == "inf_in_null_row" or not np.isfinite(wsum[wok]).all()
    gk, gsum, gok = _sort_groupby(shim, keys, v, valid, "sum")
    np.testing.assert_array_equal(gk, wk)
    np.testing.assert_array_equal(gok, wok)
    _check(gsum[wok], wsum[wok], "sort-path SUM")
    # MEAN = the SUM in the sum's type (float32 stays float32) / COUNT_VALID, one correctly rounded division in double: exactly
    # that quotient of the SUM checked above
    cnt = orc.groupby_sort_agg(keys, v, "count_valid", None, valid)[2]
    gk, gmean, gok = _sort_groupby(shim, keys, v, valid, "mean")
    np.testing.assert_array_equal(gok, wok)
    assert gmean.dtype == np.float64
    with np.errstate(invalid="ignore"):
        np.testing.assert_array_equal(gmean[wok], gsum[wok].astype(np.float64) / cnt[wok])


# ---------------------------------------------------------------------------------------------------------------------
# hash groupby SUM: global table, LDS-partitioned, auto at 600 000 rows (dense ids / sparse keys), two key columns, DataFrame
# ---------------------------------------------------------------------------------------------------------------------
def _hash_inputs(dtype, n, nkeys, nulls, seed, sparse=False, overflow=True):
    """keys in [0, nkeys) (or nkeys sparse int64 values); group 1 holds one +inf, group 2 is all positive with eight values
    whose sum leaves the range (overflow=True), group 3 holds +inf and -inf, group 4 a -inf; the rest is U[-1000, 1000)"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, nkeys, n)
    v = (rng.random(n) * 2000 - 1000).astype(dtype)
    vv = (rng.random(n) > 0.2) if nulls else None
    big = 1e308 if dtype == "float64" else 3e38
    rows = [np.nonzero(ids == g)[0] for g in range(5)]
    assert all(len(r) >= 16 for r in rows)
    v[rows[2]] = np.abs(v[rows[2]]) + v.dtype.type(1)
    special = {rows[1][len(rows[1]) // 2]: np.inf, rows[3][1]: np.inf, rows[3][-2]: -np.inf, rows[4][0]: -np.inf}
    if overflow:
        special.update({r: big for r in rows[2][:: max(1, len(rows[2]) // 8)][:8]})
    for r, x in special.items():
        v[r] = x
        if vv is not None:
            vv[r] = True
    if sparse:
        table = np.unique(rng.integers(-2**62, 2**62, 4 * nkeys))[:nkeys]
        keys = table[rng.permutation(nkeys)][ids].astype(np.int64)
    else:
        keys = ids.astype(np.int32)
    return keys, v, vv


def _groupby_raw(Column, ops, keys, vals, vv, max_groups):
    """gx_groupby_sum_count through the C ABI with the scratch kept, so that the plan's path can be read back"""
    from cudf_amd import _lib as L
    from cudf_amd.ops import _run, _dev_i64
    kc, vc = Column.from_numpy(keys), Column.from_numpy(vals, vv)
    ok, osum = Column.empty(keys.dtype, max_groups), Column.empty(vals.dtype, max_groups)
    ocv, oca = Column.empty(np.int32, max_groups), Column.empty(np.int32, max_groups)
    ng = _dev_i64()
    tmp = _run(L.lib.gx_groupby_sum_count, kc.gx, kc.data_ptr, None, vc.gx, vc.data_ptr, vc.mask_ptr if vv is not None else None,
               keys.size, max_groups, ok.data_ptr, osum.data_ptr, ocv.data_ptr, oca.data_ptr, ops.ptr(ng))
    g = int(ng.item())
    assert 0 <= g <= max_groups
    for c in (ok, osum, ocv):
        c.size = g
    info = (ctypes.c_int32 * 4)()
    L.check(L.lib.gx_groupby_plan_info(ops.ptr(tmp), max_groups, info, ops.stream_ptr()), "gx_groupby_plan_info")
    return ok.to_numpy(), osum.to_numpy(), ocv.to_numpy(), list(info)


def _check_hash(k, s, cv, keys, v, vv, what):
    o = np.argsort(k, kind="stable")
    ek, res = orc.groupby_agg(keys, v, ["sum", "count_valid"], None, vv)
    es, ev = res["sum"]
    np.testing.assert_array_equal(k[o], ek)
    np.testing.assert_array_equal(cv[o], res["count_valid"][0])
    nf = ~np.isfinite(es[ev])
    assert int(np.isposinf(es[ev]).sum()) == 2 and int(np.isneginf(es[ev]).sum()) == 1 and int(np.isnan(es[ev]).sum()) == 1, what
    assert int(nf.sum()) == 4
    _check(s[o][ev], es[ev], what)


@pytest.mark.parametrize("nulls", [False, True], ids=["nonulls", "nulls"])
@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("algo", [1, 2], ids=["global_table", "lds_partitioned"])
def test_hash_groupby_sum_non_finite_pinned_path(gx, algo, dtype, nulls):
    """gx_groupby_set_algorithm(1 | 2, 1) pins the kernels: 1 never partitions (k_aggregate: comp_add on the global table), 2 partitions every n > 0
    (k_part_fold: comp_add in LDS, on the global table for rows that spill, and in the merge)"""
    Column, ops = gx
    from cudf_amd import _lib
    keys, v, vv = _hash_inputs(dtype, N, 300, nulls, seed=7 + algo)
    _lib.lib.gx_groupby_set_algorithm(algo, 1)
    try:
        k, s, cv, _ = ops.groupby_sum_count(Column.from_numpy(keys), Column.from_numpy(v, vv), max_groups_hint=1024)
        k, s, cv = k.to_numpy(), s.to_numpy(), cv.to_numpy()
    finally:
        _lib.lib.gx_groupby_set_algorithm(0, 1)
    assert s.dtype == np.dtype(dtype)
    _check_hash(k, s, cv, keys, v, vv, f"hash groupby algo {algo}")


@pytest.mark.parametrize("path,dtype", [("dense", "float64"), ("sparse", "float64"), ("sparse", "float32")])
def test_hash_groupby_sum_non_finite_auto_path_600k(gx, path, dtype):
    """algorithm 0 past the 2^19-row threshold: the partitioned kernels, with the plan's choice read back -- dense ids by direct
    address (k_dense_aggregate; the plan that can choose them belongs to the histogram-free partition pass, which rows below
    2^22 take only with gx_groupby_set_partition_mode(2)) and sparse keys on the hash partitions."""
    Column, ops = gx
    from cudf_amd import _lib
    n = 600_000
    keys, v, vv = _hash_inputs(dtype, n, 1000, False, seed=11, sparse=path == "sparse")
    _lib.lib.gx_groupby_set_algorithm(0, 1)
    _lib.lib.gx_groupby_set_partition_mode(2 if path == "dense" else 1)
    try:
        k, s, cv, info = _groupby_raw(Column, ops, keys, v, vv, 4096)
    finally:
        _lib.lib.gx_groupby_set_partition_mode(1)
        _lib.lib.gx_groupby_set_algorithm(0, 1)
    if path == "dense":
        assert info[0] == 1 and info[1] == 0, f"the dense path was not taken / fell back ({info})"
    else:
        assert info[0] == 0, info
    _check_hash(k, s, cv, keys, v, vv, f"hash groupby auto {path}")


def test_hash_groupby_two_key_columns_non_finite(gx):
    """ops.groupby_sum_count_tables on two int32 key columns at 300 000 rows (>= 2^18: the wide-key LDS kernel, comp_add)"""
    Column, ops = gx
    n = 300_000
    keys, v, _ = _hash_inputs("float64", n, 1000, False, seed=13)
    k1, k2 = (keys // 40).astype(np.int32), (keys % 40).astype(np.int32)
    kc, s, cv, _ = ops.groupby_sum_count_tables([Column.from_numpy(k1), Column.from_numpy(k2)], Column.from_numpy(v))
    k = kc[0].to_numpy().astype(np.int64) * 40 + kc[1].to_numpy()
    _check_hash(k, s.to_numpy(), cv.to_numpy(), keys, v, None, "two key columns")


def test_dataframe_groupby_sum_mean_non_finite_matches_pandas(gx):
    """groups with +inf, -inf and both.  No overflowing group here: pandas' own Kahan sum turns a sum that overflows into NaN
    one addition later (its compensation becomes inf), so it is no reference for that case -- the oracle tests above are."""
    import pandas as pd
    import cudf_amd
    keys, v, _ = _hash_inputs("float64", N, 50, False, seed=17, overflow=False)
    exp = pd.DataFrame({"k": keys, "v": v}).groupby("k").agg(v_sum=("v", "sum"), v_mean=("v", "mean")).reset_index()
    got = cudf_amd.DataFrame({"k": keys, "v": v}).groupby("k").agg({"v": ["sum", "mean"]}).to_pandas()
    np.testing.assert_array_equal(got["k"], exp["k"])
    for c in ("v_sum", "v_mean"):
        e, g = exp[c].to_numpy(), got[c].to_numpy()
        nf = ~np.isfinite(e)
        assert int(np.isinf(e).sum()) == 2 and int(np.isnan(e).sum()) == 1
        np.testing.assert_array_equal(g[nf], e[nf])
        np.testing.assert_allclose(g[~nf], e[~nf], rtol=1e-13)  # pandas' own (Kahan) sum is the reference here


# ---------------------------------------------------------------------------------------------------------------------
# ill-conditioned sums: the compensation has to survive every boundary
# ---------------------------------------------------------------------------------------------------------------------
ILL_N = 300_007


@functools.lru_cache(maxsize=None)
def _ill_conditioned(dtype):
    """x[2j] = b_j, x[2j+1] = d_j - b_j in the column type, b_j = N(0,1) * 10^U(4,8), d_j in [0.5, 1.5): the running sum grows
    by ~1 per pair while the terms are ~1e6.  Returns (x, exact prefixes in float64, 7 contiguous group labels cut at pairs)."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(2024)
    m = (ILL_N + 1) // 2
    b = (rng.standard_normal(m) * 10.0 ** rng.uniform(4, 8, m)).astype(dt)
    d = (rng.random(m) + 0.5).astype(dt)
    x = np.empty(2 * m, dt)
    x[0::2], x[1::2] = b, d - b
    x = x[:ILL_N].copy()
    prefix = orc.exact_prefix_sums(x)
    labels = (np.arange(ILL_N) // 2 * 7 // m).astype(np.int32)  # a pair never straddles two groups
    for a in (x, prefix, labels):
        a.setflags(write=False)
    return x, prefix, labels


def _assert_separates(x, prefix, dtype):
    """The input is worth the test: plain summation in the column type fails on it, and it stays inside the conditioning of the
    1-ulp bound.  Returns the absolute slack of the few prefixes outside it: where b_j happens to cancel the running sum,
    sum|x| / |sum x| exceeds 2^50 / n and all the double-double bound gives is its absolute form n * 2^-104 * sum|x|."""
    ax = np.cumsum(np.abs(x.astype(np.float64)))
    proven = ax < np.abs(prefix) * (2.0 ** 50 / ILL_N)
    assert proven[-1] and proven.mean() > 0.999, "sum|x| / |sum x| must stay below 2^50 / n for the 1-ulp bound"
    plain = np.cumsum(x)  # sequential, in the column type
    assert plain.dtype == x.dtype
    off = _ulps(plain, _cast(prefix, dtype)) > 1
    assert off.mean() >= 0.5, f"plain cumsum is > 1 ulp off at only {off.mean():.0%} of the rows: the input no longer separates"
    return np.where(proven, 0.0, ILL_N * 2.0 ** -104 * ax)


@pytest.mark.parametrize("dtype", FLOATS)
def test_ill_conditioned_reduce_and_scan(gx, dtype):
    Column, ops = gx
    x, prefix, _ = _ill_conditioned(dtype)
    slack = _assert_separates(x, prefix, dtype)
    col = Column.from_numpy(x)
    for out_dtype in (np.float64, np.dtype(dtype).type):
        got, ok = ops.reduce(col, "sum", out_dtype)
        assert ok
        _check(np.asarray(got), _cast(prefix[-1], out_dtype), f"reduce sum -> {np.dtype(out_dtype)}")
    _check(ops.scan(col, "sum", True).to_numpy(), _cast(prefix, dtype), "inclusive scan", slack)
    _check(ops.scan(col, "sum", False).to_numpy(), _cast(np.concatenate([[0.0], prefix[:-1]]), dtype), "exclusive scan",
           np.concatenate([[0.0], slack[:-1]]))


def _ill_group_sums(x, labels, dtype):
    sums = np.array([orc.exact_sum(x[labels == g]) for g in range(7)])
    for g in range(7):  # every group is inside the conditioning of the 1-ulp bound
        assert np.abs(x[labels == g].astype(np.float64)).sum() < abs(sums[g]) * (2.0 ** 50 / ILL_N)
    return _cast(sums, dtype)


@pytest.mark.parametrize("dtype", FLOATS)
def test_ill_conditioned_sort_path_groupby(shim, dtype):  # noqa: F811
    x, prefix, labels = _ill_conditioned(dtype)
    _assert_separates(x, prefix, dtype)
    gk, gsum, gok = _sort_groupby(shim, labels, x, None, "sum")
    np.testing.assert_array_equal(gk, np.arange(7))
    assert gok.all()
    _check(gsum, _ill_group_sums(x, labels, dtype), "sort-path SUM")


@pytest.mark.parametrize("dtype", FLOATS)
@pytest.mark.parametrize("algo", [1, 2], ids=["global_table", "lds_partitioned"])
def test_ill_conditioned_hash_groupby(gx, algo, dtype):
    Column, ops = gx
    from cudf_amd import _lib
    x, prefix, labels = _ill_conditioned(dtype)
    _assert_separates(x, prefix, dtype)
    _lib.lib.gx_groupby_set_algorithm(algo, 1)
    try:
        k, s, cv, _ = ops.groupby_sum_count(Column.from_numpy(labels), Column.from_numpy(x), max_groups_hint=64)
        k, s = k.to_numpy(), s.to_numpy()
    finally:
        _lib.lib.gx_groupby_set_algorithm(0, 1)
    o = np.argsort(k)
    np.testing.assert_array_equal(k[o], np.arange(7))
    _check(s[o], _ill_group_sums(x, labels, dtype), f"hash groupby algo {algo}")
