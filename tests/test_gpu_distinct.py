"""GPU: deduplication -- ops.unique / distinct / stable_distinct / distinct_indices / distinct_count / unique_count and
DataFrame.drop_duplicates (cudf_amd/csrc/gx_distinct.hip under them).  The reference of every check is NumPy / pandas on the host
copy of the same inputs: rows get a class id from np.unique over their normalised key elements, pandas' duplicated() picks the first /
last / unduplicated row of a class.  Everything is bit-exact: the kept row numbers, and every output column against input[kept rows]
(tobytes(); validity bits and null counts included).  Row counts sit on the wave (64), chunk (4096) and table-capacity (65 536 rows:
capacity exactly 2 n; 65 537: one doubling later) edges."""
import os
import subprocess

import numpy as np
import pandas as pd
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [0, 1, 2, 63, 64, 65, 4095, 4096, 4097, 65_536, 65_537, 100_003]
KEEPS = ["any", "first", "last", "none"]


@pytest.fixture(scope="module")
def gx():
    import cudf_amd
    from cudf_amd import Column, ops
    return cudf_amd, Column, ops


# ------------------------------------------------------------------------------------------------ the reference
def _class_ids(cols, nulls_equal=True, nans_equal=True):
    """int64 class id per row over the key columns [(values, valid or None)]: equal ids <=> equal rows under the contract (null == null
    iff nulls_equal, NaN == NaN whatever sign or payload iff nans_equal, -0.0 == +0.0, a null's bytes never looked at)"""
    n = len(cols[0][0])
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    codes = np.empty((n, len(cols)), dtype=np.int64)
    alone = np.zeros(n, dtype=bool)
    for j, (v, valid) in enumerate(cols):
        isnull = np.zeros(n, dtype=bool) if valid is None else ~valid
        with np.errstate(invalid="ignore"):
            isnan = (np.isnan(v) & ~isnull) if v.dtype.kind == "f" else np.zeros(n, dtype=bool)
        ok = ~isnull & ~isnan
        c = np.full(n, -1, dtype=np.int64)
        c[isnan] = -2
        vv = v[ok]
        if v.dtype.kind == "f":
            vv = vv + v.dtype.type(0)                    # -0.0 + 0.0 = +0.0
        c[ok] = np.unique(vv, return_inverse=True)[1].reshape(-1)
        codes[:, j] = c
        if not nulls_equal:
            alone |= isnull
        if not nans_equal:
            alone |= isnan
    cls = np.unique(codes, axis=0, return_inverse=True)[1].reshape(-1).astype(np.int64)
    cls[alone] = cls.max() + 1 + np.arange(int(alone.sum()))       # a row that equals nothing is a class of its own
    return cls


def _distinct_rows(cls, keep):
    """the ascending rows distinct keeps; None under "any" (checked by its properties)"""
    if keep == "any":
        return None
    s = pd.Series(cls)
    dup = s.duplicated(keep={"first": "first", "last": "last", "none": False}[keep])
    return np.flatnonzero(~dup.to_numpy())


def _unique_rows(cls, keep):
    n = len(cls)
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    same = cls[1:] == cls[:-1]
    first = np.r_[True, ~same]
    last = np.r_[~same, True]
    return np.flatnonzero({"any": first, "first": first, "last": last, "none": first & last}[keep])


def _run(gx, fn, cols, keys, keep, **kw):
    """fn over the table cols + a row-number column; returns the kept row numbers after checking every output column against
    input[kept], bit for bit"""
    _, Column, ops = gx
    n = len(cols[0][0])
    rowid = np.arange(n, dtype=np.int32)
    out = fn([Column.from_numpy(v, valid) for v, valid in cols] + [Column.from_numpy(rowid)], keys, keep=keep, **kw)
    assert len(out) == len(cols) + 1
    kept = out[-1].to_numpy().astype(np.int64)
    assert out[-1].dtype == np.int32 and out[-1].mask is None
    assert np.all(np.diff(kept) > 0), "input order"
    assert len(kept) == 0 or (kept[0] >= 0 and kept[-1] < n)
    for o, (v, valid) in zip(out, cols):
        assert o.size == len(kept) and o.dtype == v.dtype
        assert o.to_numpy().tobytes() == v[kept].tobytes()
        ev = None if valid is None else valid[kept]
        if ev is None or ev.all():
            assert o.mask is None and o.null_count == 0
        else:
            assert o.null_count == int((~ev).sum()) and np.array_equal(o.valid_numpy(), ev)
    return kept


def _check_distinct(gx, cols, keys, keep, nulls_equal=True, nans_equal=True):
    _, _, ops = gx
    cls = _class_ids([cols[k] for k in keys], nulls_equal, nans_equal)
    kept = _run(gx, ops.distinct, cols, keys, keep, nulls_equal=nulls_equal, nans_equal=nans_equal)
    want = _distinct_rows(cls, keep)
    if want is None:                                      # KEEP_ANY: one row per class, whichever
        assert len(kept) == len(np.unique(cls)) and len(np.unique(cls[kept])) == len(kept)
    else:
        assert np.array_equal(kept, want), (keep, len(kept), len(want))
    return kept


def _check_unique(gx, cols, keys, keep, nulls_equal=True):
    _, _, ops = gx
    cls = _class_ids([cols[k] for k in keys], nulls_equal, True)
    kept = _run(gx, ops.unique, cols, keys, keep, nulls_equal=nulls_equal)
    assert np.array_equal(kept, _unique_rows(cls, keep)), keep
    return kept


# ------------------------------------------------------------------------------------------------ inputs, built once
_RNG = np.random.default_rng(20260)


def _runs(n, ndistinct):
    """int64 keys with runs of 1 .. 4 consecutive equal rows AND repeats further apart"""
    vals = _RNG.integers(-2**62, 2**62, max(ndistinct, 1), dtype=np.int64)
    picks = vals[_RNG.integers(0, len(vals), n + 4)]
    return np.repeat(picks, _RNG.integers(1, 5, n + 4))[:n].copy()


_ONE_KEY = {n: (_runs(n, max(n // 8, 1)), _RNG.integers(0, 2**31, n).astype(np.int16)) for n in ROWS}


@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("n", ROWS)
def test_distinct_one_int64_key_against_pandas(gx, n, keep):
    key, payload = _ONE_KEY[n]
    kept = _check_distinct(gx, [(key, None), (payload, None)], [0], keep)
    if keep != "any":                                     # the same through pandas' own drop_duplicates
        pdf = pd.DataFrame({"k": key, "row": np.arange(n)})
        want = pdf.drop_duplicates(subset="k", keep={"first": "first", "last": "last", "none": False}[keep])["row"].to_numpy()
        assert np.array_equal(kept, want)
    if n >= 63:                                           # the case drops something and (a class of one row may not exist) keeps something
        assert len(kept) < n and (keep == "none" or len(kept) > 0)


@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("n", ROWS)
def test_unique_one_int64_key(gx, n, keep):
    key, payload = _ONE_KEY[n]
    kept = _check_unique(gx, [(key, None), (payload, None)], [0], keep)
    if n >= 63:
        assert len(kept) < n and (keep == "none" or len(kept) > 0)
        assert not np.array_equal(kept, _distinct_rows(_class_ids([(key, None)]), "first" if keep == "any" else keep))  # unique is not distinct


_ALL_EQUAL = np.full(1 << 20, -7_000_000_007, dtype=np.int64)
_ALL_DISTINCT = _RNG.permutation(100_003).astype(np.int64) * 1_000_003
_SIXTEEN = _RNG.integers(0, 100_003 // 16, 100_003).astype(np.int64)


@pytest.mark.parametrize("keep", KEEPS)
def test_every_row_equal_contends_on_one_slot(gx, keep):
    n = len(_ALL_EQUAL)
    kept = _check_distinct(gx, [(_ALL_EQUAL, None)], [0], keep)
    assert len(kept) == (0 if keep == "none" else 1)
    if keep in ("first", "last"):
        assert kept[0] == (0 if keep == "first" else n - 1)
    ukept = _check_unique(gx, [(_ALL_EQUAL, None)], [0], keep)
    assert len(ukept) == (0 if keep == "none" else 1)


@pytest.mark.parametrize("keep", KEEPS)
def test_every_row_distinct(gx, keep):
    assert len(_check_distinct(gx, [(_ALL_DISTINCT, None)], [0], keep)) == len(_ALL_DISTINCT)
    assert len(_check_unique(gx, [(_ALL_DISTINCT, None)], [0], keep)) == len(_ALL_DISTINCT)


@pytest.mark.parametrize("keep", KEEPS)
def test_sixteen_rows_per_class(gx, keep):
    kept = _check_distinct(gx, [(_SIXTEEN, None)], [0], keep)
    if keep != "none":
        assert len(kept) == len(np.unique(_SIXTEEN))
    _check_unique(gx, [(np.sort(_SIXTEEN), None)], [0], keep)     # sorted: runs of ~16


def _mixed_table(n):
    """int8 + float64 + int32 + uint16 keys (nulls in the first two, random bytes under the nulls) and a float32 payload"""
    nan_bits = np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF7FFFFFFFFFFFF, 0x7FF8DEADBEEF0001],
                        dtype=np.uint64).view(np.float64)
    pool = np.concatenate([np.array([-0.0, 0.0, np.inf, -np.inf, 1.5, -1.5]), nan_bits])
    f = pool[_RNG.integers(0, len(pool), n)]
    fv = _RNG.random(n) < 0.8
    f[~fv] = _RNG.integers(0, 2**63, int((~fv).sum()), dtype=np.int64).view(np.float64)
    a = _RNG.integers(-1, 2, n).astype(np.int8)
    av = _RNG.random(n) < 0.8
    a[~av] = _RNG.integers(-128, 128, int((~av).sum())).astype(np.int8)
    b = _RNG.integers(0, 3, n).astype(np.int32) * 1_000_000_007
    c = _RNG.integers(65_534, 65_536, n).astype(np.uint16)
    payload = _RNG.random(n).astype(np.float32)
    pv = _RNG.random(n) < 0.9
    return [(a, av), (f, fv), (b, None), (c, None), (payload, pv)]


_MIXED = _mixed_table(20_011)


@pytest.mark.parametrize("nans_equal", [True, False])
@pytest.mark.parametrize("nulls_equal", [True, False])
@pytest.mark.parametrize("keep", KEEPS)
def test_mixed_width_keys_with_nulls_and_nans(gx, keep, nulls_equal, nans_equal):
    f = _MIXED[1][0]
    assert np.signbit(f[f == 0]).any() and not np.signbit(f[f == 0]).all() and np.isinf(f).any()
    kept = _check_distinct(gx, _MIXED, [0, 1, 2, 3], keep, nulls_equal, nans_equal)
    assert len(kept) < len(f) and (len(kept) > 0 or (keep == "none" and nulls_equal and nans_equal))
    if nans_equal:                                        # unique: NaNs always compare equal
        _check_unique(gx, _MIXED, [0, 1, 2, 3], keep, nulls_equal)
        _check_unique(gx, _MIXED, [1], keep, nulls_equal)
    _check_distinct(gx, _MIXED, [1], keep, nulls_equal, nans_equal)      # the float key alone: few classes, long contention
    _check_distinct(gx, _MIXED, [3, 0], keep, nulls_equal, nans_equal)


def test_thirty_two_key_columns(gx):
    _, Column, ops = gx
    n = 5_003
    cls = _RNG.integers(0, 64, n)
    cols = [(((cls >> (j % 6)) & 1).astype(np.int8) if j % 2 else ((cls >> (j % 6)) & 1).astype(np.int64) * -3, None) for j in range(32)]
    for keep in ("first", "none", "any"):
        kept = _check_distinct(gx, cols, list(range(32)), keep)
    assert len(np.unique(_class_ids(cols))) == 64
    with pytest.raises(ValueError):
        ops.distinct([Column.from_numpy(v) for v, _ in cols] + [Column.from_numpy(cols[0][0])], list(range(33)))


@pytest.mark.parametrize("keep", KEEPS)
def test_distinct_indices(gx, keep):
    _, Column, ops = gx
    keys = [_MIXED[k] for k in (0, 1, 2, 3)]
    for ne, na in ((True, True), (False, True), (True, False)):
        idx = ops.distinct_indices([Column.from_numpy(v, valid) for v, valid in keys], keep, ne, na)
        assert idx.dtype == np.int32 and idx.mask is None
        got = idx.to_numpy()
        cls = _class_ids(keys, ne, na)
        want = _distinct_rows(cls, keep)
        if want is None:
            assert np.all(np.diff(got) > 0) and len(got) == len(np.unique(cls)) == len(np.unique(cls[got]))
        else:
            assert np.array_equal(got, want)
    assert ops.distinct_indices([Column.from_numpy(np.zeros(0, dtype=np.int64))], keep).size == 0


# ------------------------------------------------------------------------------------------------ counts
def _column_counts(v, valid, null_policy, nan_policy):
    """(distinct_count, unique_count) of one column, restated: NAN_IS_NULL makes a NaN a null element, NAN_IS_VALID makes all NaNs
    one value; INCLUDE counts the nulls as one value, EXCLUDE never counts a null row; a run starts where a row differs from the
    physically previous row"""
    n = len(v)
    isnull = np.zeros(n, dtype=bool) if valid is None else ~valid
    with np.errstate(invalid="ignore"):
        isnan = (np.isnan(v) & ~isnull) if v.dtype.kind == "f" else np.zeros(n, dtype=bool)
    if nan_policy == "null":
        isnull, isnan = isnull | isnan, np.zeros(n, dtype=bool)
    ok = ~isnull & ~isnan
    code = np.full(n, -1, dtype=np.int64)
    code[isnan] = -2
    vv = v[ok] + v.dtype.type(0) if v.dtype.kind == "f" else v[ok]
    code[ok] = np.unique(vv, return_inverse=True)[1].reshape(-1)
    counted = np.ones(n, dtype=bool) if null_policy == "include" else ~isnull
    distinct = len(np.unique(code[counted]))
    starts = np.r_[True, code[1:] != code[:-1]] if n else np.zeros(0, dtype=bool)
    return distinct, int((starts & counted).sum())


def _count_columns():
    f, fv = _MIXED[1]
    yield "float64 with nulls and NaNs", np.sort(f[:4097]), fv[:4097]          # sorted bits: runs (NaNs of both signs at the ends)
    yield "float64 unsorted", f[:4097], fv[:4097]
    yield "[1, null, 1]", np.array([1, 99, 1], dtype=np.int32), np.array([True, False, True])
    yield "only nulls", np.arange(100, dtype=np.int64), np.zeros(100, dtype=bool)
    yield "only NaNs", np.array([np.nan, -np.nan, np.nan] * 50, dtype=np.float32), None
    yield "only NaNs, nullable", np.full(70, np.nan), _RNG.random(70) < 0.5
    yield "int16 without nulls", np.repeat(np.arange(300, dtype=np.int16), 3), None


@pytest.mark.parametrize("nan_policy", ["valid", "null"])
@pytest.mark.parametrize("null_policy", ["include", "exclude"])
def test_column_counts_under_the_policies(gx, null_policy, nan_policy):
    _, Column, ops = gx
    for name, v, valid in _count_columns():
        col = Column.from_numpy(v, valid)
        d, u = _column_counts(v, valid, null_policy, nan_policy)
        assert ops.distinct_count(col, null_policy=null_policy, nan_policy=nan_policy) == d, (name, "distinct")
        assert ops.unique_count(col, null_policy=null_policy, nan_policy=nan_policy) == u, (name, "unique")
    if (null_policy, nan_policy) == ("exclude", "valid"):
        c = Column.from_numpy(np.array([1, 99, 1], dtype=np.int32), np.array([True, False, True]))
        assert ops.unique_count(c, null_policy="exclude") == 2 and ops.distinct_count(c, null_policy="exclude") == 1
        assert _column_counts(np.array([1, 99, 1]), np.array([True, False, True]), "exclude", "valid") == (1, 2)


@pytest.mark.parametrize("nulls_equal", [True, False])
def test_table_counts(gx, nulls_equal):
    _, Column, ops = gx
    for keys in ([0, 1, 2, 3], [1], [0], [2, 3]):
        kc = [_MIXED[k] for k in keys]
        cls = _class_ids(kc, nulls_equal, True)
        cols = [Column.from_numpy(v, valid) for v, valid in kc]
        assert ops.distinct_count(cols, nulls_equal=nulls_equal) == len(np.unique(cls))
        assert ops.unique_count(cols, nulls_equal=nulls_equal) == len(_unique_rows(cls, "first"))
    assert ops.distinct_count([Column.from_numpy(np.zeros(0, dtype=np.int8))]) == 0
    assert ops.unique_count([Column.from_numpy(np.zeros(0, dtype=np.int8))]) == 0


# ------------------------------------------------------------------------------------------------ probe chains, size
_COLLIDE = (_RNG.integers(0, 300, 20_000).astype(np.int64) - 150) * 977


@pytest.mark.parametrize("keep", KEEPS)
def test_forced_collisions_probe_through_other_classes(gx, keep):
    """every row's home slot is 0: a row walks the slots of up to 299 other classes before it finds its own"""
    cudf_amd, _, _ = gx
    lib = cudf_amd._lib.lib
    assert len(np.unique(_COLLIDE)) == 300
    lib.gx_distinct_set_hash_bits(-1)
    try:
        kept = _check_distinct(gx, [(_COLLIDE, None)], [0], keep)
    finally:
        lib.gx_distinct_set_hash_bits(0)
    assert len(kept) == (300 if keep != "none" else int((np.unique(_COLLIDE, return_counts=True)[1] == 1).sum()))


_LARGE = _RNG.integers(0, 1 << 20, (1 << 22) + 4097).astype(np.int64) * 0x9E3779B1 - (1 << 50)


@pytest.mark.parametrize("keep", ["first", "none"])
def test_four_million_rows_one_million_classes(gx, keep):
    _, Column, ops = gx
    n = len(_LARGE)
    idx = ops.distinct_indices([Column.from_numpy(_LARGE)], keep).to_numpy()
    dup = pd.Series(_LARGE).duplicated(keep="first" if keep == "first" else False).to_numpy()
    assert np.array_equal(idx, np.flatnonzero(~dup))
    assert 0 < len(idx) < n


# ------------------------------------------------------------------------------------------------ DataFrame, C++
@pytest.mark.parametrize("keep", ["first", "last", False])
def test_dataframe_drop_duplicates_against_pandas(gx, keep):
    cudf_amd, Column, _ = gx
    n = 10_007
    a = _RNG.integers(0, 4, n).astype(np.int64)
    av = _RNG.random(n) < 0.7
    b = np.array([0.5, -0.0, 0.0, np.nan, -np.nan, np.inf])[_RNG.integers(0, 6, n)]
    c = _RNG.integers(0, 3, n).astype(np.int32)
    df = cudf_amd.DataFrame({"a": Column.from_numpy(a, av), "b": Column.from_numpy(b), "c": Column.from_numpy(c),
                             "row": Column.from_numpy(np.arange(n, dtype=np.int32))})
    pdf = df.to_pandas()
    assert pdf["a"].isna().any() and pdf["b"].isna().any()
    for subset in (["a", "b", "c"], ["a", "b"], "b", ["c"], None):
        got = df.drop_duplicates(subset=subset, keep=keep).to_pandas()
        want = pdf.drop_duplicates(subset=subset, keep=keep).reset_index(drop=True)
        assert list(got.columns) == list(want.columns)
        assert np.array_equal(got["row"].to_numpy(), want["row"].to_numpy()), (subset, keep)
        pd.testing.assert_frame_equal(got, want, check_dtype=False)
    assert len(df.drop_duplicates(keep=keep)) == n        # "row" is among the default subset
    with pytest.raises(ValueError):
        df.drop_duplicates(keep="any")
    with pytest.raises(KeyError):
        df.drop_duplicates(subset=["nope"])


def test_cpp_surface_runs_the_same_contract():
    """cudf::unique / distinct / stable_distinct / distinct_indices / the counts through libcudf.so: literal vectors, sliced views"""
    import __graft_entry__ as ge
    ge.build()
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "cudf_distinct_tests")], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "0 failed" in r.stdout and "[FAIL]" not in r.stdout
