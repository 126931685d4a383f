"""Pins the CPU oracle (oracle/) against the reference's own golden vectors and the published
MurmurHash3 KATs.  CPU only."""
import math
import os

import numpy as np
import pytest

from oracle import c_oracle
from oracle import cudf_oracle as orc
from tests.golden import reference_vectors as gv


@pytest.mark.parametrize("case", gv.SORT, ids=lambda c: c["name"])
def test_sort_golden(case):
    vals, mask = gv.col(case["values"], case["dtype"], case["valid"])
    got = orc.sorted_order(vals, mask, case["ascending"], case["null_before"])
    exp = np.array(case["expected"], np.int32)
    if case["compare"] == "indices":
        np.testing.assert_array_equal(got, exp)
    else:  # the reference compares gather(input, expected) with the sorted table: nulls interchangeable
        m = np.ones(len(vals), bool) if mask is None else mask
        np.testing.assert_array_equal(m[got], m[exp])
        np.testing.assert_array_equal(vals[got][m[got]], vals[exp][m[exp]])
    if mask is None:
        # keys-only sort is bit-identical to gathering through the order
        out = orc.sort_keys(vals, case["ascending"])
        assert out.tobytes() == vals[exp].tobytes()


@pytest.mark.parametrize("case", gv.SORT_TABLE, ids=lambda c: c["name"])
@pytest.mark.parametrize("dtype", ["int8", "int32", "int64", "uint16", "uint64", "float32", "float64"])
def test_sort_table_golden(case, dtype):
    cols = [np.array(c, dtype) for c in case["cols"]]
    np.testing.assert_array_equal(orc.sorted_order_table(cols, case["ascending"]), np.array(case["expected"], np.int32))
    # the lexicographic order is what LSD over the columns with the single-column oracle gives (no NaN here)
    order = np.arange(len(cols[0]))
    for c, a in reversed(list(zip(cols, case["ascending"]))):
        order = order[orc.sorted_order(c[order], None, a)]
    np.testing.assert_array_equal(order, case["expected"])


def _cols(lists, dtype):
    cols, masks = [], []
    for c in lists:
        a, m = gv.col(c, dtype)
        cols.append(a)
        masks.append(m)
    return cols, masks


@pytest.mark.parametrize("case", gv.JOIN, ids=lambda c: c["name"])
def test_join_golden(case):
    lc, lm = _cols(case["left"], case["dtype"])
    rc, rm = _cols(case["right"], case["dtype"])
    fn = {"inner": orc.inner_join, "left": orc.left_join, "full": orc.full_join}[case.get("how", "inner")]
    for eq in case["nulls_equal"]:
        l, r = fn(lc, rc, lm, rm, eq)
        if "expected_size" in case:
            assert len(l) == case["expected_size"]
        if "expected_pairs" in case:
            assert sorted(zip(l.tolist(), r.tolist())) == sorted(case["expected_pairs"])
        else:
            lp = [np.array(c) for c in case["left_payload"]]
            rp = [np.array(c) for c in case["right_payload"]]
            rows = sorted(tuple(int(c[i]) for c in lp) + tuple(int(c[j]) for c in rp)
                          for i, j in zip(l, r))
            assert rows == sorted(case["expected_rows"])


@pytest.mark.parametrize("case", gv.SEMI_ANTI, ids=lambda c: c["name"])
def test_semi_anti_golden(case):
    lc, lm = _cols(case["left"], case["dtype"])
    rc, rm = _cols(case["right"], case["dtype"])
    fn = orc.semi_join if case["how"] == "semi" else orc.anti_join
    got = fn(lc, rc, lm, rm, case["nulls_equal"])
    assert got.dtype == np.int32 and got.tolist() == case["expected"]


@pytest.mark.parametrize("case", gv.DISTINCT_JOIN, ids=lambda c: c["name"])
def test_distinct_join_golden(case):
    lc, lm = _cols(case["left"], case["dtype"])
    rc, rm = _cols(case["right"], case["dtype"])
    if case["how"] == "inner":
        l, r = orc.inner_join(lc, rc, lm, rm, True)
        assert sorted(zip(l.tolist(), r.tolist())) == sorted(case["expected_pairs"])
    else:
        assert orc.distinct_left_join(lc, rc, lm, rm, True).tolist() == case["expected"]


@pytest.mark.parametrize("vdtype", ["int32", "int64", "float64"])
@pytest.mark.parametrize("case", gv.GROUPBY, ids=lambda c: c["name"])
def test_groupby_golden(case, vdtype):
    vdtype = case.get("vals_dtype", vdtype)
    keys, km = gv.col(case["keys"], "int32", case.get("keys_valid"))
    vals, vm = gv.col(case["vals"], vdtype, case.get("vals_valid"))
    out_keys, res = orc.groupby_agg(keys, vals, [case["agg"]], km, vm, ddof=case.get("ddof", 1))
    r, rv = res[case["agg"]]
    np.testing.assert_array_equal(out_keys, np.array(case["expect_keys"], np.int32))
    ev = np.array(case["expect_valid"], bool)
    np.testing.assert_array_equal(rv, ev)
    exp = np.array(case["expect"])
    if case["agg"] == "sum":
        assert r.dtype == (np.int64 if np.dtype(vdtype).kind == "i" else np.dtype(vdtype))
    if case["agg"].startswith("count"):
        assert r.dtype == np.int32
    if case["agg"].startswith("arg"):
        assert r.dtype == np.int32
    if case["agg"] in ("mean", "var", "std"):
        assert r.dtype == np.float64
        assert np.all(orc.ulp_diff(r[ev], exp[ev].astype(np.float64)) <= 1)
    else:
        np.testing.assert_array_equal(r[ev], exp[ev].astype(r.dtype))


@pytest.mark.parametrize("vdtype", ["int32", "int64", "float64"])
@pytest.mark.parametrize("case", gv.GROUPBY_SCAN, ids=lambda c: c["name"])
def test_groupby_scan_golden(case, vdtype):
    keys, km = gv.col(case["keys"], "int32", case.get("keys_valid"))
    vals, vm = gv.col(case["vals"], vdtype, case.get("vals_valid"))
    sk, out, ov = orc.groupby_scan_sum(keys, vals, km, vm)
    np.testing.assert_array_equal(sk, np.array(case["expect_keys"], np.int32))
    ev = np.array(case["expect_valid"], bool)
    np.testing.assert_array_equal(ov, ev)
    np.testing.assert_array_equal(out[ev], np.array(case["expect"])[ev].astype(out.dtype))


@pytest.mark.parametrize("dtype", ["int8", "int32", "int64", "uint32", "float32", "float64"])
@pytest.mark.parametrize("case", gv.SCAN, ids=lambda c: c["name"])
def test_scan_golden(case, dtype):
    vals, mask = gv.col(case["values"], dtype, case["valid"])
    out, om = orc.scan(vals, case["op"], case["inclusive"], mask, case["null_include"])
    ev = np.array(case["expect_valid"], bool)
    assert out.dtype == np.dtype(dtype)
    np.testing.assert_array_equal(om, ev)
    np.testing.assert_array_equal(out[ev], np.array(case["expect"])[ev].astype(dtype))


def test_murmur3_published_kat():
    for data, seed, digest in gv.MURMUR3_KAT:
        assert orc.murmur3_32_bytes(data, seed) == digest, (data, seed)


def test_murmur3_vector_matches_scalar_and_c():
    rng = np.random.default_rng(5)
    for dt in (np.int32, np.uint32, np.int64, np.uint64, np.float32, np.float64):
        if np.dtype(dt).kind == "f":
            v = rng.standard_normal(257).astype(dt)
        else:
            info = np.iinfo(dt)
            v = rng.integers(info.min, info.max, 257, dtype=dt, endpoint=True)
        for seed in (0, 619):
            h = orc.murmur3_32(v, seed)
            ref = [orc.murmur3_32_bytes(x.tobytes(), seed) for x in v]
            np.testing.assert_array_equal(h, np.array(ref, np.uint32))
            np.testing.assert_array_equal(c_oracle.murmur3(v.view(f"u{v.dtype.itemsize}"), seed), h)
    # float normalisation: -0.0 == +0.0, every NaN payload hashes alike; nulls -> UINT32_MAX
    f = np.array([0.0, -0.0, np.nan, -np.nan], np.float64)
    h = orc.murmur3_32(f)
    assert h[0] == h[1] and h[2] == h[3]
    assert orc.murmur3_32(np.array([5], np.int32), valid=np.array([False]))[0] == 0xFFFFFFFF


def test_c_oracle_matches_numpy_oracle():
    rng = np.random.default_rng(11)
    v = rng.integers(-2**63, 2**63 - 1, 100_003, dtype=np.int64)
    v[::7] = v[3]  # duplicates
    for desc in (False, True):
        assert c_oracle.sort_i64(v, desc).tobytes() == orc.sort_keys(v, not desc).tobytes()
        np.testing.assert_array_equal(c_oracle.sorted_order_i64(v, desc), orc.sorted_order(v, None, not desc))
    for dt in (np.int32, np.uint32):  # the 32-bit keys of the cursor path's parity tests (tests/test_gpu_sort_place.py)
        ii = np.iinfo(dt)
        v32 = rng.integers(ii.min, ii.max, 100_003, dtype=dt, endpoint=True)
        v32[::5] = v32[2]
        v32[:4] = [ii.min, ii.max, 0, ii.max]
        for desc in (False, True):
            assert c_oracle.sort_32(v32, desc).tobytes() == orc.sort_keys(v32, not desc).tobytes()
    build = rng.permutation(20_000).astype(np.int64)[:5000] * 3
    probe = rng.integers(0, 60_000, 40_000).astype(np.int64)
    probe[:100] = build[:100]
    build2 = np.concatenate([build, build[:50]])  # duplicates on the build side
    l, r = c_oracle.inner_join_i64(probe, build2)
    l, r = orc.canonical_pairs(l, r)
    ol, orr = orc.inner_join(probe, build2)
    np.testing.assert_array_equal(l, ol)
    np.testing.assert_array_equal(r, orr)
    keys = rng.integers(0, 1000, 200_000).astype(np.int32)
    vals = rng.random(200_000)
    s, c = c_oracle.groupby_dense_sum_count(keys, vals, 1000)
    ok, res = orc.groupby_agg(keys, vals, ["sum", "count_valid"])
    np.testing.assert_array_equal(ok, np.arange(1000, dtype=np.int32))
    np.testing.assert_array_equal(c, res["count_valid"][0])
    assert np.all(orc.ulp_diff(s, res["sum"][0]) <= 1)  # tolerance: 1 ulp (north_star)
    x = rng.integers(-2**62, 2**62, 1000, dtype=np.int64)
    np.testing.assert_array_equal(c_oracle.inclusive_sum_i64(x), orc.scan(x, "sum")[0])


def test_descending_float_nan_block_reversed():
    # cub SortPairsDescending on the composite key (isnan*(idx+1), f): NaNs first, highest idx first
    v = np.array([1.0, np.nan, 3.0, np.nan, -np.inf, np.nan], np.float64)
    np.testing.assert_array_equal(orc.sorted_order(v, None, ascending=False), [5, 3, 1, 2, 0, 4])


def test_hash_partition_oracle_properties():
    rng = np.random.default_rng(3)
    k = rng.integers(0, 1000, 5000).astype(np.int64)
    for p in (1, 3, 8):
        order, offs = orc.hash_partition([k], p)
        assert offs[0] == 0 and offs[-1] == len(k) and len(offs) == p + 1
        pid = orc.murmur3_32(k) % np.uint32(p)
        for q in range(p):
            seg = order[offs[q]:offs[q + 1]]
            assert np.all(pid[seg] == q) and np.all(np.diff(seg) > 0)


@pytest.mark.parametrize("dtype", ["int8", "int32", "int64", "float32", "float64"])
@pytest.mark.parametrize("case", gv.REDUCE, ids=lambda c: c["name"])
def test_reduce_golden(case, dtype):
    vals, mask = gv.col(case["values"], dtype, case["valid"])
    out_dtype = (np.float64 if np.dtype(dtype).kind == "f" else np.int64) if case["op"] == "sum" else None
    r, ok = orc.reduce(vals, case["op"], mask, out_dtype)
    assert ok == case["expect_valid"]
    if ok:
        assert r == case["expect"]


@pytest.mark.parametrize("dtype", ["int32", "int64", "float32", "float64"])
@pytest.mark.parametrize("case", gv.REDUCE_INIT, ids=lambda c: c["name"])
def test_reduce_init_golden(case, dtype):
    """reduce with an initial value: the literals of reduction_tests.cpp (MinMaxReductions, Sum, Product)"""
    vals, mask = gv.col(case["values"], dtype, case["valid"])
    r, ok = orc.reduce(vals, case["op"], mask, None, init=case["init"], init_valid=case["init_valid"])
    assert ok == case["expect_valid"]
    if ok:
        assert r == case["expect"] and np.asarray(r).dtype == np.dtype(dtype)


@pytest.mark.parametrize("case", gv.REDUCE_MORE, ids=lambda c: c["name"])
def test_reduce_mean_count_any_all_golden(case):
    """cudf::reduce MEAN / COUNT_VALID / COUNT_ALL / ANY / ALL: the literals of reduction_tests.cpp (AnyAllTrueTrue, AnyAllFalseFalse,
    empty_column, Mean, Count) over the types the reference's typed tests run"""
    for dtype in case["dtypes"]:
        vals, mask = gv.col(case["values"], dtype, case["valid"])
        r, ok = orc.reduce(vals, case["op"], mask, case["out"], init=case["init"], init_valid=case["init_valid"])
        assert ok == case["expect_valid"], dtype
        if ok:
            assert r == case["expect"] and np.asarray(r).dtype == np.dtype(case["out"]), dtype


def test_reduce_more_contract():
    """what the reference throws (reductions.cpp:492-499, count.cpp:28-33, any.cu:85-86, compound.cuh:108-117)"""
    v = np.arange(5, dtype=np.int32)
    for bad in (lambda: orc.reduce(v, "mean", None, np.float64, init=1), lambda: orc.reduce(v, "count_all", None, np.int32, init=1),
                lambda: orc.reduce(v, "count_valid", None, bool), lambda: orc.reduce(v, "any", None, np.int32),
                lambda: orc.reduce(v, "mean", None, np.int32)):
        with pytest.raises(ValueError):
            bad()
    # NaN is truthy (static_cast<bool>(NaN) is true); an initial value is folded in
    assert orc.reduce(np.array([0.0, np.nan]), "any")[0] and not orc.reduce(np.array([0.0, np.nan]), "all")[0]
    assert orc.reduce(np.zeros(3, np.int32), "any", None, bool, init=7) == (True, True)
    assert orc.reduce(np.ones(3, np.int32), "all", None, bool, init=0) == (False, True)


@pytest.mark.parametrize("case", [c for c in gv.HASH_PARTITION if "throws" not in c], ids=lambda c: c["name"])
def test_hash_partition_contract_golden(case):
    """hash_partition_test.cpp: num_partitions + 1 offsets ALWAYS, the last = rows of the output; empty results"""
    cols = [np.asarray(v, dt) for dt, v in case["cols"]]
    order, offs = orc.hash_partition([cols[i] for i in case["keys"]], case["parts"], case.get("seed", 0))
    assert len(offs) == case["noffsets"] and len(order) == case["rows"]
    assert offs[0] == 0 and offs[-1] == case["rows"] and np.all(np.diff(offs) >= 0)
    if case["rows"]:
        assert np.array_equal(np.sort(order), np.arange(case["rows"]))


@pytest.mark.parametrize("map_type", ["int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64"])
@pytest.mark.parametrize("case", gv.PARTITION_BY_MAP, ids=lambda c: c["name"])
def test_partition_by_map_oracle_matches_reference(case, map_type):
    """partition_test.cpp:126-232: the literal offsets; every partition holds the reference's rows (compared as sets there)"""
    v, m = np.asarray(case["values"], np.int64), np.asarray(case["map"]).astype(map_type)
    order, offs = orc.partition_by_map(m, case["parts"])
    np.testing.assert_array_equal(offs, case["offsets"])
    exp = np.asarray(case["expected"], np.int64)
    for a, b in zip(offs[:-1], offs[1:]):
        np.testing.assert_array_equal(np.sort(v[order][a:b]), np.sort(exp[a:b]))
    assert orc.partition_by_map(m[:0], 5)[1].tolist() == [0] * 6          # :39-54 EmptyInputs


def test_identity_hash_oracle_is_the_cast_to_uint32():
    """partitioning.cu:852-872 IdentityHash: static_cast<uint32_t>(key); hash_partition_test.cpp:411-431: HASH_IDENTITY over a
    column of externally computed murmur hashes gives the offsets of hashing the columns directly"""
    assert orc.identity_hash32(np.array([-1, 5, 2**40 + 3, -2**40], np.int64)).tolist() == [0xFFFFFFFF, 5, 3, 0]
    assert orc.identity_hash32(np.array([-1, 127, -128], np.int8)).tolist() == [0xFFFFFFFF, 127, 0xFFFFFF80]
    assert orc.identity_hash32(np.array([65535, 7], np.uint16)).tolist() == [65535, 7]
    assert orc.identity_hash32(np.array([True, False])).tolist() == [1, 0]
    assert orc.identity_hash32(np.array([3.99, -0.5, -0.0, 4294967295.0], np.float64)).tolist() == [3, 0, 0, 0xFFFFFFFF]
    # outside what C++ defines: the device conversion saturates, NaN -> 0
    assert orc.identity_hash32(np.array([np.nan, -7.0, 1e20, np.inf, -np.inf], np.float32)).tolist() == [0, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0]
    assert orc.identity_hash32(np.array([9, 9], np.int32), [True, False]).tolist() == [9, 0xFFFFFFFF]
    rng = np.random.default_rng(2)
    cols = [rng.integers(-1000, 1000, 1000).astype(np.int32), rng.random(1000)]
    h = orc.row_hash(cols)
    for parts in (1, 7, 64):
        a = orc.hash_partition(cols, parts)
        b = orc.hash_partition([h], parts, hash_function="identity")
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
    two = orc.row_hash_identity([np.array([1, 2], np.int32), np.array([3, 4], np.int64)])
    assert two.tolist() == [int(orc.hash_combine(np.array([1], np.uint32), np.array([3], np.uint32))[0]),
                            int(orc.hash_combine(np.array([2], np.uint32), np.array([4], np.uint32))[0])]


# ---- round 3: the oracle restatements behind the at-scale parity tests of rank / top_k / segmented sort /
# sort-path groupby / groupby::scan COUNT / shift / replace_nulls are pinned to the reference's own literals
def test_rank_oracle_matches_every_reference_rank_vector():
    import json
    d = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "rank_vectors.json")))
    assert len(d["cases"]) == 36  # 5 methods x 6 (order, null policy, null order) + 6 percentage cases
    v = np.array(d["input"], np.int32)
    m2 = np.array(d["col2_valid"], bool)
    for c in d["cases"]:
        for col, valid in (("col1", None), ("col2", m2)):
            r, ok = orc.rank(v, valid, c["method"], not c["descending"], c["null_include"], c["null_before"], c["percentage"])
            ev, e = np.array(c[col + "_valid"], bool), np.array(c[col])
            np.testing.assert_array_equal(ok, ev, err_msg=f"{c['name']} {col} (rank_test.cpp:{c['line']})")
            np.testing.assert_allclose(r[ev], e[ev], rtol=1e-15, atol=0, err_msg=f"{c['name']} {col}")


@pytest.mark.parametrize("case", gv.GROUPBY_SORT, ids=lambda c: c["name"])
def test_groupby_sort_path_oracle_matches_reference(case):
    keys, km = gv.col(case["keys"], "int32", case.get("keys_valid"))
    for vdtype in ("int32", "int64", "float64"):
        vals, vm = gv.col(case["vals"], vdtype, case.get("vals_valid"))
        uk, ukv, out, ov = orc.groupby_sort_agg(keys, vals, case["agg"], km, vm, n_th=case.get("n", 0))
        np.testing.assert_array_equal(uk, np.array(case["expect_keys"], np.int32))
        ev = np.array(case["expect_valid"], bool)
        np.testing.assert_array_equal(ov, ev)
        np.testing.assert_array_equal(out[ev], np.array(case["expect"])[ev].astype(out.dtype))
        if case["agg"] == "product":  # integers -> int64, floats keep their type (aggregation.hpp:949-970)
            assert out.dtype == (np.float64 if vdtype == "float64" else np.int64)


@pytest.mark.parametrize("case", gv.GROUPBY_COUNT_SCAN, ids=lambda c: c["name"])
def test_groupby_count_scan_oracle_matches_reference(case):
    keys, km = gv.col(case["keys"], "int32", case.get("keys_valid"))
    vals, vm = gv.col(case["vals"], "int32", case.get("vals_valid"))
    for op, key in (("count_valid", "expect_valid_count"), ("count_all", "expect_all_count")):
        sk, out, ov = orc.groupby_scan(keys, vals, op, km, vm)
        np.testing.assert_array_equal(sk, np.array(case["expect_keys"], np.int32))
        np.testing.assert_array_equal(out, np.array(case[key], np.int32))
        assert out.dtype == np.int32 and bool(ov.all())


@pytest.mark.parametrize("case", gv.GROUPBY_SCAN, ids=lambda c: c["name"])
def test_general_groupby_scan_oracle_agrees_with_the_sum_scan_vectors(case):
    keys, km = gv.col(case["keys"], "int32", case.get("keys_valid"))
    vals, vm = gv.col(case["vals"], "int64", case.get("vals_valid"))
    sk, out, ov = orc.groupby_scan(keys, vals, "sum", km, vm)
    np.testing.assert_array_equal(sk, np.array(case["expect_keys"], np.int32))
    ev = np.array(case["expect_valid"], bool)
    np.testing.assert_array_equal(ov, ev)
    np.testing.assert_array_equal(out[ev], np.array(case["expect"])[ev])


@pytest.mark.parametrize("case", gv.GROUPBY_SHIFT, ids=lambda c: c["name"])
def test_groupby_shift_oracle_matches_reference(case):
    keys, _ = gv.col(case["keys"], "int32")
    vals, vm = gv.col(case["vals"], "int32", case.get("vals_valid"))
    _, out, ov = orc.groupby_shift(keys, vals, case["offset"], case["fill"], None, vm)
    ev = np.array(case["expect_valid"], bool)
    np.testing.assert_array_equal(ov, ev)
    np.testing.assert_array_equal(out[ev], np.array(case["expect"], np.int32)[ev])


@pytest.mark.parametrize("case", gv.GROUPBY_REPLACE_NULLS, ids=lambda c: c["name"])
def test_groupby_replace_nulls_oracle_matches_reference(case):
    keys, _ = gv.col(case["keys"], "int32")
    vals, vm = gv.col(case["vals"], "int32", case["vals_valid"])
    sk, out, ov = orc.groupby_replace_nulls(keys, vals, vm, case["following"])
    np.testing.assert_array_equal(sk, np.array(case["expect_keys"], np.int32))
    ev = np.array(case["expect_valid"], bool)
    np.testing.assert_array_equal(ov, ev)
    np.testing.assert_array_equal(out[ev], np.array(case["expect"], np.int32)[ev])


@pytest.mark.parametrize("case", gv.SEGMENTED_SORT, ids=lambda c: c["name"])
def test_segmented_sort_oracle_matches_reference(case):
    cols = [np.array(c, np.int32) for c in case["cols"]]
    order = orc.segmented_sorted_order(cols, case["offsets"], None, case["ascending"], None)
    if "expect_order" in case:
        np.testing.assert_array_equal(order, np.array(case["expect_order"], np.int32))
    if "expect_col0" in case:
        np.testing.assert_array_equal(cols[0][order], np.array(case["expect_col0"], np.int32))
    if "expect_col1" in case:
        np.testing.assert_array_equal(cols[1][order], np.array(case["expect_col1"], np.int32))


def test_top_k_and_match_count_oracles_on_the_reference_literals():
    # cpp/tests/sort/top_k_tests.cpp semantics on the vectors tests/cpp/cudf_api_tests.cpp uses
    v = np.array([7, -3, 12, 5, 12, 0, 9], np.int64)
    vals, idx, _ = orc.top_k(v, 3)
    np.testing.assert_array_equal(vals, [12, 12, 9])
    np.testing.assert_array_equal(idx, [2, 4, 6])
    np.testing.assert_array_equal(orc.top_k(v, 2, descending=False)[0], [-3, 0])
    assert len(orc.top_k(v, 0)[0]) == 0 and len(orc.top_k(v, 100)[0]) == 7
    np.testing.assert_array_equal(orc.top_k(v, 100)[1], np.arange(7))  # top_k.cu:139-145: k >= size -> iota
    vn, _, ok = orc.top_k(np.array([1.5, 9.0, 2.5, 7.0]), 2, valid=np.array([1, 0, 1, 1], bool))
    np.testing.assert_array_equal(vn, [7.0, 2.5])
    assert bool(ok.all())
    # match contexts on InnerJoinNoNulls (cpp/tests/join/join_tests.cpp:1163-1237): per-row counts add up to the pairs
    c = gv.JOIN[0]
    l, r = np.array(c["left"][0], np.int32), np.array(c["right"][0], np.int32)
    np.testing.assert_array_equal(orc.join_match_counts(l, r, "inner"), [1, 0, 2, 1, 2])
    assert int(orc.join_match_counts(l, r, "inner").sum()) == len(c["expected_rows"])
    np.testing.assert_array_equal(orc.join_match_counts(l, r, "left"), [1, 1, 2, 1, 2])


# ----------------------------------------------------------------------------------------------------------------------
# exact_sum / exact_prefix_sums: the float SUM target where plain addition gives +-inf or NaN
# ----------------------------------------------------------------------------------------------------------------------
_INF = np.inf
NONFINITE_SUMS = [  # (input, what plain left-to-right addition gives for every prefix)
    ([_INF, 1.0], [_INF, _INF]),
    ([1.0, _INF], [1.0, _INF]),
    ([-_INF, 2.0, 3.0], [-_INF, -_INF, -_INF]),
    ([1e308, 1e308], [1e308, _INF]),
    ([0.0, _INF], [0.0, _INF]),
    ([1.0, np.nan, 2.0, _INF], [1.0, np.nan, np.nan, np.nan]),
    ([2.0, _INF, 5.0, -_INF, 1.0], [2.0, _INF, _INF, np.nan, np.nan]),
    ([-1e308, -1e308, -1e308], [-1e308, -_INF, -_INF]),
]


@pytest.mark.parametrize("x,prefixes", NONFINITE_SUMS, ids=[str(c[0]) for c in NONFINITE_SUMS])
def test_exact_sum_follows_plain_addition_on_non_finite_input(x, prefixes):
    with np.errstate(over="ignore", invalid="ignore"):
        np.testing.assert_array_equal(np.cumsum(np.array(x)), prefixes)  # the table is what plain addition gives
    np.testing.assert_array_equal(orc.exact_prefix_sums(x), prefixes)
    np.testing.assert_array_equal(orc.exact_sum(x), prefixes[-1])
    for k in range(1, len(x) + 1):
        np.testing.assert_array_equal(orc.exact_sum(x[:k]), prefixes[k - 1])
    # the entry points that use the helpers
    v = np.array(x)
    np.testing.assert_array_equal(orc.reduce(v, "sum")[0], prefixes[-1])
    np.testing.assert_array_equal(orc.reduce(v, "mean")[0], prefixes[-1] / len(x))
    np.testing.assert_array_equal(orc.scan(v, "sum", exact=True)[0], prefixes)
    keys = np.zeros(len(x), np.int32)
    np.testing.assert_array_equal(orc.groupby_agg(keys, v, ["sum"])[1]["sum"][0], prefixes[-1:])
    np.testing.assert_array_equal(orc.groupby_sort_agg(keys, v, "sum")[2], prefixes[-1:])


def test_exact_sum_where_fsum_gives_up_on_a_finite_result():
    # an intermediate overflow (math.fsum raises OverflowError), widely spread exponents, subnormal results
    assert orc.exact_sum([1e308, 1e308, -1e308]) == 1e308
    np.testing.assert_array_equal(orc.exact_prefix_sums([1e308, 1e308, -1e308, -1e308]), [1e308, _INF, 1e308, 0.0])
    assert orc.exact_sum([1e300, 1e-300, -1e300]) == 1e-300
    np.testing.assert_array_equal(orc.exact_prefix_sums([1e300, 5e-324, -1e300, 5e-324]), [1e300, 1e300, 5e-324, 1e-323])
    assert orc.exact_sum([]) == 0.0 and len(orc.exact_prefix_sums([])) == 0
    # float32 outputs: past FLT_MAX the sum is inf in the output type
    v = np.full(8, 3e38, np.float32)
    assert orc.reduce(v, "sum", None, np.float32)[0] == np.float32(_INF)
    assert np.isfinite(orc.reduce(v, "sum", None, np.float64)[0])
    np.testing.assert_array_equal(orc.scan(v, "sum", exact=True)[0], np.array([3e38] + [_INF] * 7, np.float32))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_exact_sum_matches_fsum_on_finite_input(seed):
    rng = np.random.default_rng(seed)
    for n in (1, 2, 17, 1000, 50_000):
        x = rng.standard_normal(n) * 10.0 ** rng.uniform(-30, 30, n)
        x[rng.random(n) < 0.1] = 0.0
        want = math.fsum(x)
        assert orc.exact_sum(x) == want
        assert orc.exact_sum(x.astype(np.float32)) == math.fsum(x.astype(np.float32).astype(np.float64))
        assert orc.exact_prefix_sums(x)[-1] == want
        assert orc._scaled_int_to_float(*orc._exact_total_int(x)) == want  # the path taken when fsum overflows


def test_exact_prefix_sums_match_rational_arithmetic():
    """Every prefix against fractions.Fraction (float(Fraction) is correctly rounded): 20 000 ill-conditioned rows (pairs
    b, d - b: the running sum is ~1e7 times smaller than the terms), a wide-exponent column, and -- the size the GPU tests use --
    300 007 rows checked at every 97th prefix with math.fsum.  CPU time measured: exact_prefix_sums 0.2 s at 300 007 rows (a plain
    Fraction loop over as many: about 3 s); the whole test about 1.5 s."""
    from fractions import Fraction
    rng = np.random.default_rng(3)
    b = rng.standard_normal(10_000) * 10.0 ** rng.uniform(4, 8, 10_000)
    x = np.empty(20_000)
    x[0::2], x[1::2] = b, (rng.random(10_000) + 0.5) - b
    wide = rng.standard_normal(3000) * 10.0 ** rng.uniform(-300, 300, 3000)
    for col in (x, wide, x.astype(np.float32)):
        got = orc.exact_prefix_sums(col)
        f = Fraction(0)
        want = np.empty(len(col))
        for i, v in enumerate(col.tolist()):
            f += Fraction(v)
            want[i] = float(f)
        np.testing.assert_array_equal(got, want)
    big = rng.standard_normal(300_007) * 10.0 ** rng.uniform(-5, 8, 300_007)
    got = orc.exact_prefix_sums(big)
    for k in range(96, 300_007, 97 * 40):
        assert got[k] == math.fsum(big[: k + 1])
    assert got[-1] == math.fsum(big)


# ----------------------------------------------------------------------------------------------------------------------
# float MIN / MAX / ARGMIN / ARGMAX with NaN: one order on every entry point (the row comparator's: every NaN is one value
# above +inf, NaN == NaN; nulls never take part).  Inputs and expected outputs are typed out by hand.
#   MIN: the smallest non-NaN valid value, NaN only when every valid value is NaN.   MAX: NaN once a valid value is NaN.
#   ARGMIN / ARGMAX: the smallest row among those equal to that extreme.
#   cummin: NaN until the first non-NaN valid value, then the running minimum of the non-NaN values.   cummax: NaN from
#   the first NaN onward.   Exclusive scans show the identity +-inf in row 0.
# ----------------------------------------------------------------------------------------------------------------------
_N = np.nan
_T, _F = True, False


def _odd_nans(dtype):
    """-NaN and a NaN with a signalling-looking payload (quiet bit clear), made from their bits"""
    if np.dtype(dtype) == np.float64:
        return np.array([0xFFF8000000000000, 0x7FF0000000000001], np.uint64).view(np.float64)
    return np.array([0xFFC00000, 0x7F800001], np.uint32).view(np.float32)


# (name, values, valid or None, MIN, MAX, ARGMIN, ARGMAX, result valid, inclusive cummin, inclusive cummax); "-N" / "sN" are
# replaced by the two NaNs of _odd_nans; values under a null (valid False) are unspecified and written as 0
NAN_EXTREMES = [
    ("nan_hides_nothing", [1.0, _N, 0.5], None, 0.5, _N, 2, 1, _T, [1.0, 1.0, 0.5], [1.0, _N, _N]),
    ("null_then_nan", [7.0, _N], [_F, _T], _N, _N, 1, 1, _T, [0, _N], [0, _N]),
    ("nan_then_null", [_N, 7.0], [_T, _F], _N, _N, 0, 0, _T, [_N, 0], [_N, 0]),
    ("null_nan_null", [9.0, _N, 9.0], [_F, _T, _F], _N, _N, 1, 1, _T, [0, _N, 0], [0, _N, 0]),
    ("one_nan", [_N], None, _N, _N, 0, 0, _T, [_N], [_N]),
    ("all_nan", [_N, _N, _N], None, _N, _N, 0, 0, _T, [_N, _N, _N], [_N, _N, _N]),
    ("all_null", [3.0, _N], [_F, _F], 0, 0, 0, 0, _F, [0, 0], [0, 0]),
    ("leading_nan", [_N, 2.0, _N, 1.0], None, 1.0, _N, 3, 0, _T, [_N, 2.0, 2.0, 1.0], [_N, _N, _N, _N]),
    ("trailing_nan", [3.0, 1.0, _N], None, 1.0, _N, 1, 2, _T, [3.0, 1.0, 1.0], [3.0, 3.0, _N]),
    ("interior_nan", [2.0, _N, 5.0, 1.0], None, 1.0, _N, 3, 1, _T, [2.0, 2.0, 2.0, 1.0], [2.0, _N, _N, _N]),
    ("nan_and_inf", [np.inf, _N, np.inf], None, np.inf, _N, 0, 1, _T, [np.inf, np.inf, np.inf], [np.inf, _N, _N]),
    ("odd_nans", ["-N", 4.0, "sN", -np.inf, np.inf], None, -np.inf, _N, 3, 0, _T,
     [_N, 4.0, 4.0, -np.inf, -np.inf], [_N, _N, _N, _N, _N]),
    ("odd_nans_only", ["sN", "-N"], None, _N, _N, 0, 0, _T, [_N, _N], [_N, _N]),
    ("null_between", [5.0, 0.0, _N, 6.0], [_T, _F, _T, _T], 5.0, _N, 0, 2, _T, [5.0, 0, 5.0, 5.0], [5.0, 0, _N, _N]),
]


def _nan_case(case, dtype):
    name, vals, valid, mn, mx, amin, amax, ok, cmin, cmax = case
    odd = _odd_nans(dtype)
    v = np.array([_N if isinstance(x, str) else x for x in vals], dtype)
    u = odd.view(f"u{odd.itemsize}")
    for i, x in enumerate(vals):  # as bits: a scalar on its way through a Python float may lose its payload
        if isinstance(x, str):
            v.view(u.dtype)[i] = u[0 if x == "-N" else 1]
            assert np.isnan(v[i]) and v.view(u.dtype)[i] == u[0 if x == "-N" else 1]
    m = None if valid is None else np.array(valid, bool)
    return v, m, mn, mx, amin, amax, ok, np.array(cmin, dtype), np.array(cmax, dtype)


def _same(got, want, where=None):
    """equal values with NaN == NaN (any payload), and the same dtype"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    if where is not None:
        got, want = got[where], want[where]
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("case", NAN_EXTREMES, ids=[c[0] for c in NAN_EXTREMES])
def test_float_extremes_nan_rule_one_column(case, dtype):
    v, m, mn, mx, amin, amax, ok, cmin, cmax = _nan_case(case, dtype)
    sel = np.ones(len(v), bool) if m is None else m
    dt = np.dtype(dtype).type
    # reduce
    for op, want in (("min", mn), ("max", mx)):
        r, rok = orc.reduce(v, op, m)
        assert rok == ok
        if ok:
            _same(r, dt(want))
    # one group: hash-path and sort-path aggregations
    keys = np.full(len(v), 4, np.int32)
    _, res = orc.groupby_agg(keys, v, ["min", "max", "argmin", "argmax"], None, m)
    for agg, want in (("min", mn), ("max", mx)):
        assert res[agg][1].tolist() == [ok]
        _, _, so, sok = orc.groupby_sort_agg(keys, v, agg, None, m)
        assert sok.tolist() == [ok]
        if ok:
            _same(res[agg][0], np.array([want], dtype))
            _same(so, np.array([want], dtype))
    for agg, want in (("argmin", amin), ("argmax", amax)):
        assert res[agg][1].tolist() == [ok]
        if ok:
            _same(res[agg][0], np.array([want], np.int32))
    # scans: inclusive, and the exclusive one is the inclusive one shifted behind the identity
    for op, want, ident in (("min", cmin, np.inf), ("max", cmax, -np.inf)):
        out, om = orc.scan(v, op, True, m)
        np.testing.assert_array_equal(om, sel)
        _same(out, want, sel)
        exc, em = orc.scan(v, op, False, m)
        np.testing.assert_array_equal(em, sel)
        assert exc[0] == dt(ident) and exc.dtype == v.dtype
        _, gout, gm = orc.groupby_scan(keys, v, op, None, m)
        np.testing.assert_array_equal(gm, sel)
        _same(gout, want, sel)


def test_float_extremes_nan_rule_exclusive_scan_and_null_include():
    v = np.array([_N, 2.0, _N, 1.0])
    _same(orc.scan(v, "min", False)[0], np.array([np.inf, _N, 2.0, 2.0]))
    _same(orc.scan(v, "max", False)[0], np.array([-np.inf, _N, _N, _N]))
    v = np.array([3.0, 1.0, _N, 0.5], np.float32)
    _same(orc.scan(v, "min", False)[0], np.array([np.inf, 3.0, 1.0, 1.0], np.float32))
    _same(orc.scan(v, "max", False)[0], np.array([-np.inf, 3.0, 3.0, _N], np.float32))
    # a null before the NaN: the rows behind it still see the identity, then the NaN, then the number
    v, m = np.array([5.0, _N, 1.0, 8.0]), np.array([_F, _T, _T, _T])
    out, om = orc.scan(v, "min", False, m)
    assert om.tolist() == [_F, _T, _T, _T]
    _same(out[1:], np.array([np.inf, _N, 1.0]))
    out, om = orc.scan(v, "max", False, m)
    _same(out[1:], np.array([-np.inf, _N, _N]))
    # null_policy::INCLUDE: everything from the first null on is null (one row later in an exclusive scan); the values do not change
    v, m = np.array([_N, 4.0, 0.0, _N]), np.array([_T, _T, _F, _T])
    out, om = orc.scan(v, "min", True, m, null_include=True)
    assert om.tolist() == [_T, _T, _F, _F]
    _same(out[:2], np.array([_N, 4.0]))
    out, om = orc.scan(v, "max", False, m, null_include=True)
    assert om.tolist() == [_T, _T, _T, _F]
    _same(out[:3], np.array([-np.inf, _N, _N]))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_float_extremes_nan_rule_groups(dtype):
    """four groups in one table, keys unsorted: {1, NaN, 0.5}, {null, NaN}, {NaN, NaN, NaN}, {null, null}"""
    keys = np.array([30, 10, 20, 10, 40, 30, 10, 30, 20, 40], np.int32)
    vals = np.array([_N, 1.0, 0.0, _N, 0.0, _N, 0.5, _N, _N, 0.0], dtype)
    valid = np.array([_T, _T, _F, _T, _F, _T, _T, _T, _T, _F])
    want_valid = [_T, _T, _T, _F]
    uk, res = orc.groupby_agg(keys, vals, ["min", "max", "argmin", "argmax"], None, valid)
    assert uk.tolist() == [10, 20, 30, 40]
    for agg, want in (("min", [0.5, _N, _N]), ("max", [_N, _N, _N])):
        assert res[agg][1].tolist() == want_valid
        _same(res[agg][0][:3], np.array(want, dtype))
        for keys_sorted in (False, True):
            o = np.argsort(keys, kind="stable") if keys_sorted else np.arange(len(keys))
            sk, _, so, sok = orc.groupby_sort_agg(keys[o], vals[o], agg, None, valid[o], False, keys_sorted)
            assert sk.tolist() == [10, 20, 30, 40] and sok.tolist() == want_valid
            _same(so[:3], np.array(want, dtype))
    assert res["argmin"][1].tolist() == want_valid and res["argmax"][1].tolist() == want_valid
    _same(res["argmin"][0][:3], np.array([6, 8, 0], np.int32))  # rows of the ORIGINAL table; the first NaN row of a NaN extreme
    _same(res["argmax"][0][:3], np.array([3, 8, 0], np.int32))
    # groupby::scan: rows in sorted-key order (stable): 10: [1, NaN, 0.5]  20: [null, NaN]  30: [NaN, NaN, NaN]  40: [null, null]
    sel = np.array([_T, _T, _T, _F, _T, _T, _T, _T, _F, _F])
    for op, want in (("min", [1.0, 1.0, 0.5, 0, _N, _N, _N, _N, 0, 0]), ("max", [1.0, _N, _N, 0, _N, _N, _N, _N, 0, 0])):
        sk, out, om = orc.groupby_scan(keys, vals, op, None, valid)
        assert sk.tolist() == [10, 10, 10, 20, 20, 30, 30, 30, 40, 40]
        np.testing.assert_array_equal(om, sel)
        _same(out, np.array(want, dtype), sel)
    # a group's running minimum does not leak into the next one
    sk, out, _ = orc.groupby_scan(np.array([1, 0, 1, 0], np.int32), np.array([_N, _N, 3.0, 2.0], dtype), "min")
    _same(out, np.array([_N, 2.0, _N, 3.0], dtype))
    sk, out, _ = orc.groupby_scan(np.array([1, 0, 1, 0], np.int32), np.array([3.0, _N, _N, 2.0], dtype), "max")
    _same(out, np.array([_N, _N, 3.0, _N], dtype))


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_float_scan_oracles_unchanged_on_nan_free_input(dtype):
    """the scan oracles before the NaN rule: numpy's accumulate over the identity-filled column, pandas' grouped cummin / cummax"""
    import pandas as pd
    rng = np.random.default_rng(5)
    n = 5000
    v = (rng.standard_normal(n) * 100).astype(dtype)
    v[rng.integers(0, n, 40)] = rng.choice(np.array([np.inf, -np.inf, 0.0, -0.0], dtype), 40)
    keys = rng.integers(0, 9, n).astype(np.int32)
    for m in (None, rng.random(n) > 0.2):
        for op, f, ident in (("min", np.minimum.accumulate, np.inf), ("max", np.maximum.accumulate, -np.inf)):
            x = v if m is None else np.where(m, v, np.dtype(dtype).type(ident)).astype(dtype)
            for inclusive in (True, False):
                want = f(x) if inclusive else np.concatenate([np.array([ident], dtype), f(x)[:-1]])
                got, _ = orc.scan(v, op, inclusive, m)
                assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
            o = np.argsort(keys, kind="stable")
            gb = pd.Series(x[o]).groupby(keys[o])
            want = (gb.cummin() if op == "min" else gb.cummax()).to_numpy().astype(dtype)
            _, got, _ = orc.groupby_scan(keys, v, op, None, m)
            assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
