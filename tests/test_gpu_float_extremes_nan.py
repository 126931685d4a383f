"""GPU: float MIN / MAX / ARGMIN / ARGMAX with NaN on every entry point -- one order everywhere.

The rule (oracle/cudf_oracle.py: sortable_bits, float_running_extreme; literal vectors in tests/test_oracle_golden.py) is the row
comparator's order: every NaN is one value above +inf and equal to every other NaN, -0.0 == +0.0, nulls never take part.
  MIN: the smallest non-NaN valid value, NaN only when every valid value is NaN.   MAX: NaN once a valid value is NaN.
  ARGMIN / ARGMAX: the smallest row among those equal to that extreme.
  cummin: NaN until the first non-NaN valid value, then the running minimum of the non-NaN values; cummax: NaN from the first
  NaN onward; an exclusive scan shows +-inf in row 0.

Entry points: ops.reduce, ops.scan (inclusive / exclusive, null_include both ways), ops.groupby_min_max and
ops.groupby_argmin_argmax (global table, LDS-partitioned, the auto path at 2^19 rows), cudf::groupby::aggregate MIN / MAX / ARGMIN /
ARGMAX through the C++ shim on the hash path and on the sort path (keys unsorted and sorted::YES), groupby::scan MIN / MAX, and
ops.rolling_window as the cross-check that the five families agree on one input.

Comparison: exact.  After mapping every NaN to one NaN, values, validity and dtype equal the oracle's, in every group and row
(a value under a null is unspecified and not compared; zeros compare by value: the sign of a zero result is unspecified).

Inputs are placements, not random sprinkling: a wrong operator goes wrong by POSITION.  The kernels built on gx_scan.hpp walk
a 4096-row chunk (SCAN_CHUNK) with four waves, a wave covering 1024 consecutive rows as 16 steps (SCAN_IPT) of 64 rows: row r
of a wave is lane r % 64 of step r / 64.  The lanes of a step are combined by a tree with offsets 1, 2, 4, 8, 16 and 32, the
steps in order, the waves in order, the chunks by a scan of their partials; the look-back scan (ops.scan MIN / MAX) does the same in
tiles of 16384 rows (LB_BT * SCAN_IPT) and reads 16 predecessors per look-back round.  Every segment below holds one NaN and one
true extreme on opposite sides of one such boundary, once with the NaN before the extreme and once after it.  A segment is a
group of the groupby tables (laid out so that its first row has the alignment the placement needs) and a column of its own for
reduce / scan.  With nulls, every fifth background row is null and holds a NaN or a value beyond the extreme underneath.

The NaNs themselves vary: any NaN equals any NaN, so every placed NaN and every NaN under a null is written from its bits, cycling
through the quiet NaN, -NaN, a payload with the quiet bit clear and the all-ones pattern (NAN_BITS), from a start that differs
between segments, layouts and null variants.  A kernel that tells NaN from number by anything but "is not equal to itself" -- a
sign, a high word, one bit pattern kept for a marker, as FloatMin (gx_common.hpp) does after rewriting every NaN it loads -- meets
the NaNs that break it.
"""
import ctypes
import functools
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cudf_oracle as orc
from tests.test_gpu_cpp_parity import Dev, Out, NPT, shim  # noqa: F401  (the shim fixture and the device-column helpers)

KIND = dict(min=3, max=4, argmax=16, argmin=17)  # cudf::aggregation::Kind
FLOATS = ["float64", "float32"]
WAVE = 64              # lanes
STEP_ROWS = 64         # element k of a lane is 64 rows after element k - 1
WAVE_ROWS = 1024       # SCAN_IPT * 64
CHUNK = 4096           # SCAN_CHUNK
LB_TILE = 16384        # LB_BT * SCAN_IPT
LB_WIN = 16
ARG_FILL = 0x7F7F7F7F  # what gx_groupby_arg_select leaves for a group in which no row equals the extreme
SIZES = [1, 2, 3, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 17]
EXT = {"min": -5.0, "max": 5000.0}        # the true extreme of a segment; the background is 10 .. 1009
BEYOND = {"min": -1e30, "max": 1e30}      # under a null: would win if a null took part
# Any NaN equals any NaN: the quiet NaN numpy writes, -NaN, a payload with the quiet bit clear, and all ones below the sign -- the
# last is, in float64, the very pattern FloatMin (gx_common.hpp) keeps for "nothing yet"; float32 NaNs keep sign and payload
# through the kernels' widening to double
NAN_BITS = {"float64": np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0x7FFFFFFFFFFFFFFF], np.uint64),
            "float32": np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF], np.uint32)}


def _write_nans(v, rows, start):
    """v[rows[j]] = the NaN NAN_BITS[(start + j) % 4], as bits"""
    pat = NAN_BITS[v.dtype.name]
    v.view(pat.dtype)[rows] = pat[(start + np.arange(len(rows))) % len(pat)]
    assert np.isnan(v[rows]).all()


@pytest.fixture(scope="module")
def gx():
    import torch
    assert torch.cuda.is_available()
    import cudf_amd  # noqa: F401
    from cudf_amd import Column, ops
    return Column, ops


# ---------------------------------------------------------------------------------------------------------------------
# segments
# ---------------------------------------------------------------------------------------------------------------------
class Seg:
    """n rows; NaN at `nan`, the extreme at `ext` (None: none), designed nulls at `nulls`; `align`: what the first row's index is a
    multiple of in a table; `inf`: the extreme is -inf / +inf instead of EXT; `sprinkle`: takes background nulls in the null variant"""

    def __init__(self, name, n, align=1, nan=(), ext=None, nulls=(), inf=False, sprinkle=True):
        self.name, self.n, self.align, self.nan, self.ext, self.nulls, self.inf, self.sprinkle = name, n, align, list(nan), ext, list(nulls), inf, sprinkle
        assert all(0 <= p < n for p in self.nan + self.nulls + ([] if ext is None else [ext]))
        assert ext is None or (ext not in self.nan and ext not in self.nulls)

    def build(self, op, with_nulls, dtype):
        """(values of dtype, valid) -- None when the segment needs nulls and the variant has none.  The NaNs are written as bits,
        cycling through NAN_BITS from a start that changes with the segment, the operator and the variant"""
        if self.nulls and not with_nulls:
            return None
        i = np.arange(self.n)
        v = (10.0 + (i * 37 % 1000)).astype(dtype)
        valid = np.ones(self.n, bool)
        if with_nulls and self.sprinkle and self.n >= 64:
            valid[i % 5 == 3] = False
        valid[self.nan] = True
        valid[self.nulls] = False  # (a designed null may sit on a NaN: the NaN is then only the bytes under it)
        if self.ext is not None:
            v[self.ext] = (-np.inf if op == "min" else np.inf) if self.inf else EXT[op]
            valid[self.ext] = True
        under = np.nonzero(~valid)[0]
        v[under[1::2]] = BEYOND[op]
        nan_rows = np.concatenate([np.asarray(self.nan, np.int64), under[0::2]])
        start = zlib.crc32(self.name.encode()) + (op == "max") + 2 * with_nulls
        _write_nans(v, nan_rows, start)
        return v, valid


def _pairs(name, n, align, a, b, **kw):
    """the NaN before the extreme, and after it"""
    return [Seg(f"{name}_nan_first", n, align, nan=[a], ext=b, **kw), Seg(f"{name}_ext_first", n, align, nan=[b], ext=a, **kw)]


def _segments():
    s = []
    # lane-tree offsets 1, 2, 4, 8 (inside a row of 16 lanes), 16, 32 (across rows), and neighbours across the row borders
    for a, b in [(3, 4), (3, 5), (3, 7), (3, 11), (5, 21), (5, 37), (15, 16), (31, 32), (0, 63)]:
        s += _pairs(f"lanes_{a}_{b}", WAVE, WAVE, a, b, inf=(b - a == 2))
    # steps of one wave: the same lane one step later, far steps with the lanes crossed, first row against last row
    s += _pairs("step_0_1", WAVE_ROWS, WAVE_ROWS, 5, STEP_ROWS + 5)
    s += _pairs("step_3_12", WAVE_ROWS, WAVE_ROWS, 3 * STEP_ROWS + 40, 12 * STEP_ROWS + 2, inf=True)
    s += _pairs("step_first_last", WAVE_ROWS, WAVE_ROWS, 0, WAVE_ROWS - 1)
    # two waves of one chunk
    s += _pairs("waves_near", 2 * WAVE_ROWS, 2 * WAVE_ROWS, 1000, 1030)
    s += _pairs("waves_far", 2 * WAVE_ROWS, 2 * WAVE_ROWS, 10, 2040, inf=True)
    # two chunks
    s += _pairs("chunks_near", 2 * CHUNK, CHUNK, CHUNK - 6, CHUNK + 4)
    s += _pairs("chunks_far", 2 * CHUNK, CHUNK, 100, 8000)
    # the scan of the chunk partials: three whole chunks between the two
    s += _pairs("partials", 5 * CHUNK, CHUNK, 77, 4 * CHUNK + 900, inf=True)
    # three chunks, one NaN in the middle one, the extreme in the first or in the last
    s.append(Seg("three_chunks_ext_first", 3 * CHUNK, CHUNK, nan=[CHUNK + 2000], ext=50))
    s.append(Seg("three_chunks_ext_last", 3 * CHUNK, CHUNK, nan=[CHUNK + 2000], ext=2 * CHUNK + 4000))
    # small groups wherever they fall
    s.append(Seg("one_nan", 1, nan=[0]))
    s.append(Seg("one_number", 1, ext=0))
    s.append(Seg("all_nan", 70, nan=range(70), sprinkle=False))
    s.append(Seg("nan_then_number", 2, nan=[0], ext=1))
    s.append(Seg("inf_nan_inf", 3, nan=[1], ext=0, inf=True))
    s.append(Seg("null_nan", 2, nan=[1], nulls=[0]))
    s.append(Seg("nan_null", 2, nan=[0], nulls=[1]))
    s.append(Seg("null_nan_null", 3, nan=[1], nulls=[0, 2]))
    s.append(Seg("nulls_around_only_nan", 200, nan=[150], nulls=[p for p in range(200) if p != 150], sprinkle=False))
    s.append(Seg("all_null", 3, nulls=[0, 1, 2]))
    s.append(Seg("all_null_130", 130, nulls=range(130), sprinkle=False))
    s.append(Seg("all_nan_but_last", 130, nan=range(129), ext=129, sprinkle=False))
    # an unaligned group over four chunks
    n = 3 * CHUNK + 17
    s += _pairs("unaligned", n, 1, n // 2, n - 1)
    return s


def _column_segments():
    """reduce / scan only: the sizes at which the kernels change shape, and the tiles of the look-back scan"""
    s = []
    for n in SIZES:
        s.append(Seg(f"n{n}_all_nan", n, nan=range(n), sprinkle=False))
        if n == 1:
            continue
        s += _pairs(f"n{n}_ends", n, 1, 0, n - 1, inf=(n % 2 == 1))
        if n >= 3:
            s += _pairs(f"n{n}_middle", n, 1, n // 2 - 1, n // 2)
    s += _pairs("lb_tiles_near", 2 * LB_TILE, 1, LB_TILE - 4, LB_TILE + 6)
    s += _pairs("lb_tiles_far", 5 * LB_TILE + 17, 1, 100, 4 * LB_TILE + 5, inf=True)
    s += _pairs("lb_past_window", (LB_WIN + 2) * LB_TILE + 1, 1, 7, (LB_WIN + 1) * LB_TILE + 3)  # the first round cannot reach tile 0
    return s


@functools.lru_cache(maxsize=None)
def _columns(dtype, op, with_nulls):
    """[(name, values, valid or None)]: every segment as a column of its own"""
    out = []
    for seg in _segments() + _column_segments():
        b = seg.build(op, with_nulls, dtype)
        if b is not None:
            out.append((seg.name, b[0], b[1] if with_nulls else None))
    return out


@functools.lru_cache(maxsize=None)
def _table(dtype, op, with_nulls, pad_to=0):
    """(keys int32, values, valid or None, first rows): the segments as the groups of one table, keys ascending, every segment's first
    row aligned as it asks (plain groups fill the gaps).  pad_to: further groups of 37 rows with a NaN each, up to that many rows."""
    keys, vals, valid, starts = [], [], [], {}
    pos, key = 0, 1

    def put(v, m):
        nonlocal pos, key
        keys.append(np.full(len(v), key, np.int32))
        vals.append(v)
        valid.append(m)
        pos += len(v)
        key += 3

    for seg in _segments():
        b = seg.build(op, with_nulls, dtype)
        if b is None:
            continue
        gap = -pos % seg.align
        if gap:
            put((10.0 + np.arange(gap) % 900).astype(dtype), np.ones(gap, bool))
        assert pos % seg.align == 0
        starts[seg.name] = pos
        put(*b)
    while pos < pad_to:
        m = min(37, pad_to - pos)
        v = (10.0 + (np.arange(m) * 11 + key) % 900).astype(dtype)
        _write_nans(v, np.array([key % m]), key)
        put(v, np.arange(m) % 4 != 1 if with_nulls else np.ones(m, bool))
    keys, vals, valid = np.concatenate(keys), np.concatenate(vals), np.concatenate(valid)
    assert vals.dtype == np.dtype(dtype)
    assert with_nulls or valid.all()
    return keys, vals, (valid if with_nulls else None), starts


def _riffle(keys, vals, valid):
    """the rows of a key-sorted table in a random order that keeps every group's own row order: a stable sort by key gives the
    table back, so each group meets the kernels at the positions it was laid out for"""
    rng = np.random.default_rng(7)
    o = np.argsort(keys[rng.permutation(len(keys))], kind="stable")
    uk, uv = np.empty_like(keys), np.empty_like(vals)
    uk[o], uv[o] = keys, vals
    um = None
    if valid is not None:
        um = np.empty_like(valid)
        um[o] = valid
    assert (uk[np.argsort(uk, kind="stable")] == keys).all() and not (uk == keys).all()
    return uk, uv, um


def _same(got, want, valid=None, what=""):
    """the oracle's dtype and values, NaN == NaN whatever its sign and payload; `valid`: the rows that hold a value"""
    got, want = np.array(got, copy=True), np.array(want, copy=True)
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if valid is not None:
        got, want = got[valid], want[valid]
    if got.dtype.kind == "f":
        got[np.isnan(got)] = np.nan
        want[np.isnan(want)] = np.nan
    np.testing.assert_array_equal(got, want, err_msg=what)


def test_the_placements_are_what_the_docstring_says():
    """CPU check of the test's own inputs: a NaN and an extreme per placement, on opposite sides of the boundary, in both orders;
    the alignment holds in the tables; the oracle gives the designed answer"""
    segs = {s.name: s for s in _segments()}
    for a, b in [(3, 4), (3, 5), (3, 7), (3, 11), (5, 21), (5, 37)]:
        for order in ("nan_first", "ext_first"):
            s = segs[f"lanes_{a}_{b}_{order}"]
            assert abs(s.nan[0] - s.ext) == b - a in (1, 2, 4, 8, 16, 32) and (s.nan[0] < s.ext) == (order == "nan_first")
    s = segs["step_0_1_nan_first"]
    assert s.ext - s.nan[0] == STEP_ROWS and s.ext // WAVE_ROWS == s.nan[0] // WAVE_ROWS
    s = segs["waves_near_nan_first"]
    assert s.nan[0] // WAVE_ROWS != s.ext // WAVE_ROWS and s.nan[0] // CHUNK == s.ext // CHUNK
    s = segs["chunks_near_ext_first"]
    assert s.nan[0] // CHUNK == s.ext // CHUNK + 1
    s = segs["partials_nan_first"]
    assert s.ext // CHUNK - s.nan[0] // CHUNK - 1 >= 3
    s = segs["three_chunks_ext_last"]
    assert s.n == 3 * CHUNK and s.nan[0] // CHUNK == 1 and s.ext // CHUNK == 2
    for dtype in FLOATS:  # the one NaN of a placement is a different bit pattern in each of the four tables, all four in turn
        u = NAN_BITS[dtype].dtype
        for name in ("lanes_3_4_nan_first", "partials_ext_first", "one_nan"):
            seen = set()
            for with_nulls in (False, True):
                for op in ("min", "max"):
                    v, _ = segs[name].build(op, with_nulls, dtype)
                    seen.add(int(v.view(u)[segs[name].nan[0]]))
            assert seen == set(NAN_BITS[dtype].tolist()), (name, dtype)
        v, m = segs["all_nan"].build("min", True, dtype)
        assert set(v.view(u).tolist()) == set(NAN_BITS[dtype].tolist()) and m.all()
    for with_nulls in (False, True):
        for op in ("min", "max"):
            keys, vals, valid, starts = _table("float64", op, with_nulls)
            assert len(keys) < 160_000 and (np.diff(keys) >= 0).all()
            for name, p in starts.items():
                assert p % segs[name].align == 0 and (p == 0 or keys[p] != keys[p - 1])
            uk, res = orc.groupby_agg(keys, vals, [op], None, valid)
            r, ok = res[op]
            for name, p in starts.items():
                s, g = segs[name], int(np.searchsorted(uk, keys[p]))
                if all(q in s.nulls for q in range(s.n)):
                    assert not ok[g], name
                elif op == "max" and any(q not in s.nulls for q in s.nan):
                    assert ok[g] and np.isnan(r[g]), name
                elif s.ext is not None:
                    assert ok[g] and r[g] == ((-np.inf if op == "min" else np.inf) if s.inf else EXT[op]), name
                elif s.nan:
                    assert ok[g] and np.isnan(r[g]), name  # MIN of NaN alone


# ---------------------------------------------------------------------------------------------------------------------
# ops.reduce / ops.scan: every segment as a column
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_nulls", [False, True], ids=["no_nulls", "nulls"])
@pytest.mark.parametrize("op", ["min", "max"])
@pytest.mark.parametrize("dtype", FLOATS)
def test_reduce_min_max_with_nan(gx, dtype, op, with_nulls):
    Column, ops = gx
    for design in ("min", "max"):  # (a column laid out for MAX is one more input for MIN, and the other way round)
        for name, v, m in _columns(dtype, design, with_nulls):
            got, ok = ops.reduce(Column.from_numpy(v, m), op)
            want, wok = orc.reduce(v, op, m)
            assert ok == wok, (name, design)
            if wok:
                _same(got, want, None, f"reduce {op} of {name} ({design} layout, n={len(v)})")


@pytest.mark.parametrize("with_nulls", [False, True], ids=["no_nulls", "nulls"])
@pytest.mark.parametrize("op", ["min", "max"])
@pytest.mark.parametrize("dtype", FLOATS)
def test_scan_min_max_with_nan(gx, dtype, op, with_nulls):
    Column, ops = gx
    for name, v, m in _columns(dtype, "min", with_nulls) + _columns(dtype, "max", with_nulls):  # both layouts: other NaN patterns
        col = Column.from_numpy(v, m)
        for inclusive in (True, False):
            for null_include in (False, True):
                out = ops.scan(col, op, inclusive, null_include)
                want, wm = orc.scan(v, op, inclusive, m, null_include)
                what = f"scan {op} of {name} (n={len(v)}, inclusive={inclusive}, null_include={null_include})"
                if m is None:
                    assert out.mask is None, what
                else:
                    np.testing.assert_array_equal(out.valid_numpy(), wm, err_msg=what)
                _same(out.to_numpy(), want, wm, what)
                if not inclusive and wm[0]:
                    assert out.to_numpy()[0] == (np.inf if op == "min" else -np.inf), what


# ---------------------------------------------------------------------------------------------------------------------
# hash groupby (ops): global table, LDS partitions, the auto path at 2^19 rows
# ---------------------------------------------------------------------------------------------------------------------
def _check_hash_groupby(Column, ops, keys, vals, valid, what):
    K, V = Column.from_numpy(keys), Column.from_numpy(vals, valid)
    ek, res = orc.groupby_agg(keys, vals, ["min", "max", "argmin", "argmax", "count_valid"], None, valid)
    k, mn, mx, cv = ops.groupby_min_max(K, V, max_groups_hint=1024)
    o = np.argsort(k.to_numpy(), kind="stable")
    np.testing.assert_array_equal(k.to_numpy()[o], ek, err_msg=what)
    np.testing.assert_array_equal(cv.to_numpy()[o], res["count_valid"][0], err_msg=what)
    has = res["min"][1]
    np.testing.assert_array_equal(has, res["count_valid"][0] > 0)
    _same(mn.to_numpy()[o], res["min"][0], has, what + " MIN")
    _same(mx.to_numpy()[o], res["max"][0], has, what + " MAX")
    k2, amin, amax, cv2 = ops.groupby_argmin_argmax(K, V)
    o = np.argsort(k2.to_numpy(), kind="stable")
    np.testing.assert_array_equal(k2.to_numpy()[o], ek, err_msg=what)
    np.testing.assert_array_equal(cv2.to_numpy()[o], res["count_valid"][0], err_msg=what)
    for got, agg in ((amin, "argmin"), (amax, "argmax")):
        g = got.to_numpy()[o]
        assert (g[has] != ARG_FILL).all(), f"{what} {agg}: a group in which no row equals its extreme"
        _same(g, res[agg][0], has, f"{what} {agg}")


@pytest.mark.parametrize("algo", [1, 2], ids=["global_table", "lds_partitions"])
@pytest.mark.parametrize("with_nulls", [False, True], ids=["no_nulls", "nulls"])
@pytest.mark.parametrize("dtype", FLOATS)
def test_hash_groupby_min_max_argmin_argmax_with_nan(gx, dtype, with_nulls, algo):
    Column, ops = gx
    from cudf_amd import _lib
    _lib.lib.gx_groupby_set_algorithm(algo, 1)
    try:
        for design in ("min", "max"):
            keys, vals, valid, _ = _table(dtype, design, with_nulls)
            _check_hash_groupby(Column, ops, *_riffle(keys, vals, valid), f"hash groupby algo {algo} ({design} layout)")
    finally:
        _lib.lib.gx_groupby_set_algorithm(0, 1)


@pytest.mark.parametrize("with_nulls", [False, True], ids=["no_nulls", "nulls"])
@pytest.mark.parametrize("dtype", FLOATS)
def test_hash_groupby_auto_path_at_the_partitioning_threshold(gx, dtype, with_nulls):
    """2^19 rows: the smallest table the auto path hands to the LDS-partitioned kernels (PART_MIN_ROWS, gx_groupby.hip)"""
    Column, ops = gx
    from cudf_amd import _lib
    _lib.lib.gx_groupby_set_algorithm(0, 1)
    try:
        keys, vals, valid, _ = _table(dtype, "min", with_nulls, 1 << 19)
        assert len(keys) == 1 << 19
        _check_hash_groupby(Column, ops, *_riffle(keys, vals, valid), "hash groupby, auto path at 2^19 rows")
    finally:
        _lib.lib.gx_groupby_set_algorithm(0, 1)


# ---------------------------------------------------------------------------------------------------------------------
# cudf::groupby::aggregate and groupby::scan through the C++ shim
# ---------------------------------------------------------------------------------------------------------------------
def _aggregate(shim_call, keys, vals, valid, agg, force_sort, keys_sorted):
    """(keys, result, result valid) of cudf::groupby::aggregate, groups in ascending key order"""
    n = len(keys)
    dk, dv = Dev(keys), Dev(vals, valid)
    ok_, ov = Out(np.int32, n, True), Out(np.float64, n, True)
    kn, vn, g, vt = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    # force_sort = 1: a second NTH_ELEMENT request keeps the request off the hash path
    shim_call("shim_groupby_aggregate", dk.tid, dk.p, dk.mp, dk.nulls, dv.tid, dv.p, dv.mp, dv.nulls, n, KIND[agg], 0, 0,
              1 if keys_sorted else 0, 1 if force_sort else 0, ok_.p, ok_.mp, ctypes.byref(kn), ov.p, ov.mp, ctypes.byref(vn),
              ctypes.byref(g), ctypes.byref(vt))
    G = g.value
    k, r, rv = ok_.get(G), ov.get(G, NPT[vt.value]), ov.valid(G)
    if force_sort:
        assert (np.diff(k) > 0).all(), "the sort path returns its groups in key order"
    o = np.argsort(k, kind="stable")
    return k[o], r[o], rv[o]


def _check_aggregate(shim_call, keys, vals, valid, force_sort, keys_sorted, what):
    ek, res = orc.groupby_agg(keys, vals, ["min", "max", "argmin", "argmax"], None, valid)
    for agg in ("min", "max", "argmin", "argmax"):
        k, r, rv = _aggregate(shim_call, keys, vals, valid, agg, force_sort, keys_sorted)
        want, wv = res[agg]
        if force_sort and agg in ("min", "max"):  # the sort path has an oracle of its own; the two agree (test_oracle_golden.py)
            sk, _, want, wv = orc.groupby_sort_agg(keys, vals, agg, None, valid, False, keys_sorted)
            np.testing.assert_array_equal(sk, ek)
        np.testing.assert_array_equal(k, ek, err_msg=f"{what} {agg}")
        np.testing.assert_array_equal(rv, wv, err_msg=f"{what} {agg}: validity")
        if agg.startswith("arg"):
            assert (r[wv] != ARG_FILL).all(), f"{what} {agg}: a group in which no row equals its extreme"
        _same(r, want, wv, f"{what} {agg}")


@pytest.mark.parametrize("path", ["hash", "sort", "sort_presorted"])
@pytest.mark.parametrize("with_nulls", [False, True], ids=["no_nulls", "nulls"])
@pytest.mark.parametrize("dtype", FLOATS)
def test_cpp_groupby_aggregate_with_nan(shim, dtype, with_nulls, path):  # noqa: F811
    for design in ("min", "max"):
        keys, vals, valid, _ = _table(dtype, design, with_nulls)
        if path != "sort_presorted":
            keys, vals, valid = _riffle(keys, vals, valid)
        _check_aggregate(shim, keys, vals, valid, path != "hash", path == "sort_presorted", f"{path} path ({design} layout)")


@pytest.mark.parametrize("dtype", FLOATS)
def test_cpp_groupby_hash_and_sort_paths_agree(shim, dtype):  # noqa: F811
    """the same request with and without the NTH_ELEMENT aggregation that moves it to the sort path: identical results"""
    for design in ("min", "max"):
        keys, vals, valid = _riffle(*_table(dtype, design, True)[:3])
        for agg in ("min", "max", "argmin", "argmax"):
            hk, hr, hv = _aggregate(shim, keys, vals, valid, agg, False, False)
            sk, sr, sv = _aggregate(shim, keys, vals, valid, agg, True, False)
            np.testing.assert_array_equal(hk, sk)
            np.testing.assert_array_equal(hv, sv, err_msg=f"{agg}: validity differs between the paths")
            _same(hr, sr, sv, f"{agg} ({design} layout): hash path against sort path")


@pytest.mark.parametrize("keys_sorted", [False, True], ids=["unsorted", "presorted"])
@pytest.mark.parametrize("with_nulls", [False, True], ids=["no_nulls", "nulls"])
@pytest.mark.parametrize("dtype", FLOATS)
def test_cpp_groupby_scan_min_max_with_nan(shim, dtype, with_nulls, keys_sorted):  # noqa: F811
    for op in ("min", "max"):
        keys, vals, valid, _ = _table(dtype, op, with_nulls)
        if not keys_sorted:
            keys, vals, valid = _riffle(keys, vals, valid)
        n = len(keys)
        dk, dv = Dev(keys), Dev(vals, valid)
        ok_, ov = Out(np.int32, n), Out(dtype, n, True)
        vn, rows, vt = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        shim("shim_groupby_scan", dk.tid, dk.p, dk.mp, dk.nulls, dv.tid, dv.p, dv.mp, dv.nulls, n, KIND[op], 0, 1 if keys_sorted else 0,
             ok_.p, ov.p, ov.mp, ctypes.byref(vn), ctypes.byref(rows), ctypes.byref(vt))
        wk, want, wv = orc.groupby_scan(keys, vals, op, None, valid, False, keys_sorted)
        assert rows.value == n == len(wk)
        np.testing.assert_array_equal(ok_.get(n), wk)
        np.testing.assert_array_equal(ov.valid(n), wv)
        assert vn.value == int((~wv).sum())
        _same(ov.get(n, NPT[vt.value]), want, wv, f"groupby::scan {op}")


# ---------------------------------------------------------------------------------------------------------------------
# the five families on one input
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", FLOATS)
def test_reduce_scan_groupby_rolling_agree_on_one_input(gx, shim, dtype):  # noqa: F811
    """One key-sorted table with nulls (the groups of up to 1024 rows): a group's MIN / MAX from ops.reduce and the last row of
    ops.scan over its rows, from the hash groupby, from the sort-path groupby, from the last valid row of groupby::scan, and from a
    grouped rolling window that spans the group -- all equal to the oracle's, hence to each other; the running extremes of groupby::scan and
    of a rolling window that looks back over the whole group agree row by row."""
    Column, ops = gx
    keys, vals, valid = [], [], []
    for j, seg in enumerate(s for s in _segments() if s.n <= WAVE_ROWS):
        v, m = seg.build("min" if j % 2 else "max", True, dtype)
        keys.append(np.full(seg.n, 5 * j + 2, np.int32))
        vals.append(v)
        valid.append(m)
    keys, vals, valid = np.concatenate(keys), np.concatenate(vals), np.concatenate(valid)
    n, span = len(keys), WAVE_ROWS
    K, V = Column.from_numpy(keys), Column.from_numpy(vals, valid)
    for op in ("min", "max"):
        ek, res = orc.groupby_agg(keys, vals, [op], None, valid)
        want, has = res[op]
        bounds = np.searchsorted(keys, np.append(ek, keys[-1] + 1))
        # reduce and scan, group by group
        for g in range(len(ek)):
            lo, hi = bounds[g], bounds[g + 1]
            r, ok = ops.reduce(Column.from_numpy(vals[lo:hi], valid[lo:hi]), op)
            assert ok == has[g]
            if ok:
                _same(r, want[g], None, f"reduce {op}, group {g}")
                last = ops.scan(Column.from_numpy(vals[lo:hi], valid[lo:hi]), op, True).to_numpy()[-1]
                _same(last, want[g], None, f"last row of scan {op}, group {g}")
        # hash groupby
        k, mn, mx, cv = ops.groupby_min_max(K, V, max_groups_hint=1024)
        o = np.argsort(k.to_numpy(), kind="stable")
        np.testing.assert_array_equal(cv.to_numpy()[o] > 0, has)
        _same((mn if op == "min" else mx).to_numpy()[o], want, has, f"hash groupby {op}")
        # sort-path groupby
        sk, sr, sv = _aggregate(shim, keys, vals, valid, op, True, True)
        np.testing.assert_array_equal(sv, has)
        _same(sr, want, has, f"sort-path groupby {op}")
        # groupby::scan: the last valid row of a group holds the group's extreme
        run, rv = orc.groupby_scan(keys, vals, op, None, valid, False, True)[1:]
        got_run = ops.groupby_scan(K, V, op).to_numpy()
        _same(got_run, run, rv, f"groupby::scan {op}")
        for g in np.nonzero(has)[0]:
            last_valid = bounds[g] + int(np.nonzero(valid[bounds[g]:bounds[g + 1]])[0][-1])
            _same(got_run[last_valid], want[g], None, f"last valid row of groupby::scan {op}, group {g}")
        # rolling: a window over the whole group, and one that looks back over the whole group (the running extreme)
        whole = ops.rolling_window(V, span, span, 1, op, [K])
        wvalid = whole.valid_numpy() if whole.mask is not None else np.ones(n, bool)
        labels = np.searchsorted(ek, keys)
        np.testing.assert_array_equal(wvalid, has[labels])
        _same(whole.to_numpy(), want[labels], wvalid, f"rolling {op} over the group")
        back = ops.rolling_window(V, span, 0, 1, op, [K])
        bvalid = back.valid_numpy() if back.mask is not None else np.ones(n, bool)
        both = bvalid & rv
        assert both.sum() > n // 2
        _same(back.to_numpy(), run, both, f"rolling {op} looking back against groupby::scan")
