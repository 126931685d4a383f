"""GPU: the spill path of the LDS-partitioned single-key groupby (k_part_fold in cudf_amd/csrc/gx_groupby.hip).

A workgroup folds the rows of one hash partition into an open-addressing table in LDS and stops inserting new keys at 7/8 load; a
row whose key finds no slot after that goes to the global table one by one, and at the end the LDS-resident partial groups are
merged into the same global table.  The other groupby tests never fill a table that far (at 512 partitions their densest case puts
about 3900 groups into tables of 4864-6656 slots), so here every key comes from ONE partition: 9000 distinct keys (+ one hot key
among them, + the all-ones key, which lives in the dedicated slot of another partition) against tables of at most 6656 slots, one
workgroup per (partition, split).  Groups then exist half in LDS and half in the global table and have to meet there."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cudf_oracle as orc

N = 600_000
POOL = 9000
PART = 137                      # the 9-bit partition every pool key hashes to
MAX_GROUPS_HINT = 1 << 14
LDS_BUDGET = 160 * 1024 - 2048  # gx_groupby.hip


def _lds_slots(slot_bytes):
    return (LDS_BUDGET // slot_bytes) // 256 * 256


# slots per LDS table: key + the aggregate's words (SUM: sum, compensation, count_valid [+ count_all with value nulls];
# MIN / MAX: min, max, count_valid)
SLOTS = {("sum", ksz, nulls): _lds_slots(ksz + 8 + 8 + 4 + (4 if nulls else 0)) for ksz in (4, 8) for nulls in (False, True)}
SLOTS.update({("minmax", ksz, nulls): _lds_slots(ksz + 8 + 8 + 4) for ksz in (4, 8) for nulls in (False, True)})


def _lds_nsub(max_groups, slots, pbits=9):
    """lds_nsub of gx_groupby.hip: workgroups per (partition, split)"""
    per_part = max(max_groups, 1) / float(1 << pbits)
    nsub = 1
    while nsub < 16 and per_part / nsub > 0.65 * slots:
        nsub *= 2
    return nsub


def _partition(k):
    """part_hash >> 55: ((k + 1) * 0x9E3779B97F4A7C15 mod 2^64) >> 55"""
    with np.errstate(over="ignore"):
        return ((np.asarray(k).astype(np.int64).view(np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)) >> np.uint64(55)


@functools.lru_cache(maxsize=None)
def _rows(nulls):
    """keys (int64; every value fits int32), key validity, value validity -- shared by every case"""
    cand = np.arange(1, 6_000_000, dtype=np.int64)
    pool = cand[_partition(cand) == PART][:POOL]
    assert len(pool) == POOL
    rng = np.random.default_rng(77)
    keys = pool[rng.integers(0, POOL, N)]
    keys[1::3] = pool[11]       # a hot key on a third of the rows
    keys[::97] = -1             # the all-ones key: the dedicated slot
    kv = (rng.random(N) > 0.03) if nulls else None
    vv = (rng.random(N) > 0.2) if nulls else None
    if nulls:
        vv[keys == pool[7]] = False  # a group with only null values keeps its slot, count 0
    for a in (keys, kv, vv):
        if a is not None:
            a.setflags(write=False)
    return keys, kv, vv


@functools.lru_cache(maxsize=None)
def _values(vdtype):
    rng = np.random.default_rng(78)
    if vdtype == "sum_float64":
        vals = rng.random(N) * 2000.0 - 700.0
    elif vdtype == "sum_int64":
        vals = rng.integers(-2**62, 2**62, N).astype(np.int64)
    elif vdtype == "mm_float64":
        vals = rng.random(N) * 2000.0 - 1000.0
        vals[::50] = -0.0
        vals[1::97] = np.inf
        vals[3::1013] = -np.inf
        vals[7::211] = np.nan
    else:
        vals = rng.integers(-2**15, 2**15 - 1, N, dtype=np.int16, endpoint=True)
    vals.setflags(write=False)
    return vals


@functools.lru_cache(maxsize=None)
def _expected(nulls, vkind):
    keys, kv, vv = _rows(nulls)
    aggs = ["sum", "count_valid", "count_all"] if vkind.startswith("sum") else ["min", "max", "count_valid"]
    return orc.groupby_agg(keys, _values(vkind), aggs, kv, vv)


@pytest.fixture(scope="module")
def gx():
    import torch
    assert torch.cuda.is_available()
    import cudf_amd  # noqa: F401
    from cudf_amd import Column, ops
    return Column, ops


def _check_reaches_the_spill(agg, kdtype, nulls):
    """what the test claims: one workgroup per (partition, split), and more distinct keys in its partition than 7/8 of ANY table size"""
    keys, kv, _ = _rows(nulls)
    live = keys if kv is None else keys[kv]
    distinct = np.unique(live[_partition(live) == PART]).size
    assert distinct > max(SLOTS.values()) * 7 // 8
    s = SLOTS[(agg, np.dtype(kdtype).itemsize, nulls)]
    assert distinct > s - s // 8                        # MAXKEYS of this case's table
    assert _lds_nsub(min(N, MAX_GROUPS_HINT), s) == 1


@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("vkind", ["sum_float64", "sum_int64"])
@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("kdtype", ["int32", "int64"])
def test_sum_count_when_the_lds_table_spills(gx, kdtype, nulls, vkind, nsplit):
    Column, ops = gx
    from cudf_amd import _lib
    _check_reaches_the_spill("sum", kdtype, nulls)
    keys, kv, vv = _rows(nulls)
    vals = _values(vkind)
    ek, res = _expected(nulls, vkind)
    _lib.lib.gx_groupby_set_algorithm(2, nsplit)
    try:
        k, s, cv, ca = ops.groupby_sum_count(Column.from_numpy(keys.astype(kdtype), kv), Column.from_numpy(vals, vv),
                                             max_groups_hint=MAX_GROUPS_HINT)
    finally:
        _lib.lib.gx_groupby_set_algorithm(0, 1)
    o = np.argsort(k.to_numpy(), kind="stable")
    assert k.to_numpy().dtype == np.dtype(kdtype)
    np.testing.assert_array_equal(k.to_numpy()[o], ek)
    np.testing.assert_array_equal(cv.to_numpy()[o], res["count_valid"][0])
    np.testing.assert_array_equal(ca.to_numpy()[o], res["count_all"][0])
    es, ev = res["sum"]
    got = s.to_numpy()[o]
    if vkind == "sum_int64":
        assert got.dtype == np.int64
        np.testing.assert_array_equal(got[ev], es[ev])
    else:
        assert np.all(orc.ulp_diff(got[ev], es[ev]) <= 1), "f64 SUM must be within 1 ulp of the exact sum"
    if nulls:
        assert not ev.all()  # the group whose values are all null is there


@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("vkind", ["mm_float64", "mm_int16"])
@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("kdtype", ["int32", "int64"])
def test_min_max_when_the_lds_table_spills(gx, kdtype, nulls, vkind, nsplit):
    Column, ops = gx
    from cudf_amd import _lib
    _check_reaches_the_spill("minmax", kdtype, nulls)
    keys, kv, vv = _rows(nulls)
    vals = _values(vkind)
    ek, res = _expected(nulls, vkind)
    _lib.lib.gx_groupby_set_algorithm(2, nsplit)
    try:
        k, mn, mx, cv = ops.groupby_min_max(Column.from_numpy(keys.astype(kdtype), kv), Column.from_numpy(vals, vv),
                                            max_groups_hint=MAX_GROUPS_HINT)
    finally:
        _lib.lib.gx_groupby_set_algorithm(0, 1)
    o = np.argsort(k.to_numpy(), kind="stable")
    np.testing.assert_array_equal(k.to_numpy()[o], ek)
    np.testing.assert_array_equal(cv.to_numpy()[o], res["count_valid"][0])
    emn, ev = res["min"]
    emx, _ = res["max"]
    assert mn.to_numpy().dtype == vals.dtype
    np.testing.assert_array_equal(mn.to_numpy()[o][ev], emn[ev])   # -0.0 == +0.0 and NaN == NaN under array_equal
    np.testing.assert_array_equal(mx.to_numpy()[o][ev], emx[ev])
    if nulls:
        assert not ev.all()
