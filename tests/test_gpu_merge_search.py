"""GPU: cudf::merge and cudf::lower_bound / upper_bound -- ops.merge_order / merge_sorted / lower_bound / upper_bound,
DataFrame.searchsorted and the C ABI under them (cudf_amd/csrc/gx_merge.hip).  The reference of every check is the oracle's
lexicographic row comparator, oracle.sorted_order_rows: inputs are made sorted with it per table, the expected merge map is its
stable order of the concatenation a || b (bit-exact), the expected bounds come from its order of needles || haystack (lower) and
haystack || needles (upper).  Row counts are sized from gx_merge_tile_rows(), so the tile edges stay on the tested shapes."""
import ctypes
import os
import subprocess
import zlib

import numpy as np
import pytest

from oracle import cudf_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (na, nb) as functions of the tile T
PAIRS = {
    "0,0": lambda T: (0, 0), "0,5": lambda T: (0, 5), "5,0": lambda T: (5, 0), "1,1": lambda T: (1, 1),
    "T-1,1": lambda T: (T - 1, 1), "T,T": lambda T: (T, T), "T+1,T-1": lambda T: (T + 1, T - 1),
    "3T+7,1": lambda T: (3 * T + 7, 1), "1,3T+7": lambda T: (1, 3 * T + 7), "2^20+3,2^19-5": lambda T: (2**20 + 3, 2**19 - 5),
}
SHAPES = ["all_equal", "a_below_b", "b_below_a", "keys_0_8", "random64"]
DTYPES = ["int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float32", "float64", "bool"]


@pytest.fixture(scope="module")
def gx():
    import cudf_amd
    from cudf_amd import Column, ops
    return cudf_amd, Column, ops


@pytest.fixture(scope="module")
def T(gx):
    return int(gx[0]._lib.lib.gx_merge_tile_rows())


def _per(v, k):
    return [v] * k if isinstance(v, bool) else list(v)


def _sort_table(cols, valids, asc, nbf):
    """the table's rows brought into the order under test (by the oracle)"""
    if len(cols[0]) == 0:
        return cols, valids
    o = orc.sorted_order_rows(cols, valids, asc, nbf)
    return [c[o] for c in cols], [None if v is None else v[o] for v in valids]


def _concat(a_cols, a_valids, b_cols, b_valids):
    cols = [np.concatenate([x, y]) for x, y in zip(a_cols, b_cols)]
    valids = []
    for x, y, vx, vy in zip(a_cols, b_cols, a_valids, b_valids):
        if vx is None and vy is None:
            valids.append(None)
        else:
            valids.append(np.concatenate([np.ones(len(x), bool) if vx is None else vx, np.ones(len(y), bool) if vy is None else vy]))
    return cols, valids


def _expected_map(a_cols, a_valids, b_cols, b_valids, asc, nbf):
    cols, valids = _concat(a_cols, a_valids, b_cols, b_valids)
    if len(cols[0]) == 0:
        return np.zeros(0, np.int32)
    return orc.sorted_order_rows(cols, valids, asc, nbf)


def _upload(Column, cols, valids):
    return [Column.from_numpy(c, v) for c, v in zip(cols, valids)]


def _check_merge(gx, a_cols, b_cols, asc=True, nbf=True, a_valids=None, b_valids=None, presorted=False):
    _, Column, ops = gx
    k = len(a_cols)
    a_valids = a_valids or [None] * k
    b_valids = b_valids or [None] * k
    asc, nbf = _per(asc, k), _per(nbf, k)
    if not presorted:
        a_cols, a_valids = _sort_table(a_cols, a_valids, asc, nbf)
        b_cols, b_valids = _sort_table(b_cols, b_valids, asc, nbf)
    got = ops.merge_order(_upload(Column, a_cols, a_valids), _upload(Column, b_cols, b_valids), asc, nbf).to_numpy()
    want = _expected_map(a_cols, a_valids, b_cols, b_valids, asc, nbf)
    assert got.dtype == np.int32 and got.tobytes() == want.astype(np.int32).tobytes(), \
        f"first difference at {int(np.flatnonzero(got != want)[0]) if len(got) == len(want) else 'length'}"
    return a_cols, a_valids, b_cols, b_valids, got


def _keys(shape, na, nb, rng):
    if shape == "all_equal":
        return np.full(na, 42, np.int64), np.full(nb, 42, np.int64)
    if shape == "a_below_b":
        return rng.integers(-1000, 0, na).astype(np.int64), rng.integers(0, 1000, nb).astype(np.int64)
    if shape == "b_below_a":
        return rng.integers(0, 1000, na).astype(np.int64), rng.integers(-1000, 0, nb).astype(np.int64)
    if shape == "keys_0_8":
        return rng.integers(0, 8, na).astype(np.int64), rng.integers(0, 8, nb).astype(np.int64)
    return rng.integers(-2**63, 2**63 - 1, na, dtype=np.int64), rng.integers(-2**63, 2**63 - 1, nb, dtype=np.int64)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("pair", list(PAIRS))
def test_merge_map_on_the_tile_edges(gx, T, pair, shape):
    """all rows equal puts the tie rule across every tile and thread boundary; the other shapes move the splits to the ends and into
    the middle of the tiles"""
    na, nb = PAIRS[pair](T)
    a, b = _keys(shape, na, nb, np.random.default_rng(zlib.crc32(f"{pair}/{shape}".encode())))
    _check_merge(gx, [a], [b])


def _float_specials(dt, n, rng):
    u = np.uint32 if dt == np.float32 else np.uint64
    nan_bits = {np.float32: [0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FC12345],
                np.float64: [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF, 0x7FF8000000012345]}[dt]
    pool = np.concatenate([np.array([0.0, -0.0, np.inf, -np.inf, 1.5, -1.5, 1e-30, -1e-30], dt), np.array(nan_bits, u).view(dt)])
    v = rng.standard_normal(n).astype(dt)
    pick = rng.random(n) < 0.6
    v[pick] = pool[rng.integers(0, len(pool), int(pick.sum()))]
    return v


def _column(dtype, n, rng, few=True):
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return _float_specials(dt.type, n, rng)
    if dt.kind == "b":
        return rng.integers(0, 2, n).astype(bool)
    info = np.iinfo(dt)
    if few:
        pool = np.array([info.min, info.min + 1, -1 if info.min < 0 else 1, 0, 1, 2, info.max - 1, info.max], dt)
        return pool[rng.integers(0, len(pool), n)]
    return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)


@pytest.mark.parametrize("ascending", [True, False])
@pytest.mark.parametrize("dtype", DTYPES)
def test_merge_map_for_every_key_dtype(gx, T, dtype, ascending):
    """the extremes of every integer type; floats with +-0, +-inf and NaNs of both signs and several payloads (all NaNs tie)"""
    rng = np.random.default_rng(DTYPES.index(dtype) * 2 + ascending)
    _check_merge(gx, [_column(dtype, T + 1, rng)], [_column(dtype, 2 * T - 1, rng)], ascending)
    _check_merge(gx, [_column(dtype, 777, rng, few=False)], [_column(dtype, T + 5, rng, few=False)], ascending)


@pytest.mark.parametrize("spec", [
    (("int8", "float64"), (True, False)),
    (("float32", "uint16"), (False, True)),
    (("int64", "int8", "float32"), (True, False, True)),
    (("bool", "uint64", "int16"), (False, False, True)),
], ids=lambda s: "-".join(f"{d}{'+' if a else '-'}" for d, a in zip(*s)))
def test_merge_map_with_several_key_columns(gx, T, spec):
    """two and three key columns of mixed widths and directions; few values per column, so ties run deep into the columns behind"""
    dtypes, asc = spec
    rng = np.random.default_rng(len(dtypes) * 7 + sum(asc))
    for na, nb in ((T + 1, T - 1), (3 * T + 7, 2 * T + 1)):
        _check_merge(gx, [_column(d, na, rng) for d in dtypes], [_column(d, nb, rng) for d in dtypes], list(asc))


def test_merge_map_with_32_key_columns(gx, T):
    rng = np.random.default_rng(32)
    dts = [DTYPES[k % len(DTYPES)] for k in range(32)]
    asc = [bool(k % 3) for k in range(32)]

    def table(n):
        return [(rng.integers(0, 2, n) * (1 if k < 28 else rng.integers(1, 3, n))).astype(dts[k]) for k in range(32)]

    _check_merge(gx, table(T + 9), table(2 * T - 3), asc)


@pytest.mark.parametrize("ascending", [True, False])
@pytest.mark.parametrize("null_before", [True, False])
@pytest.mark.parametrize("dtype", ["int32", "float64", "int8", "uint16"])
def test_merge_map_with_nullable_keys(gx, T, dtype, null_before, ascending):
    """nulls tie with each other and sit where null_before and the direction put them; the bytes under a null are random"""
    rng = np.random.default_rng(DTYPES.index(dtype) * 4 + 2 * null_before + ascending)
    for na, nb, pa, pb in ((T + 1, T - 1, 0.3, 0.3), (5, 3 * T + 7, 1.0, 0.5), (T, 100, 0.0, 0.2)):
        a, b = _column(dtype, na, rng), _column(dtype, nb, rng)
        va, vb = rng.random(na) >= pa, rng.random(nb) >= pb
        _check_merge(gx, [a], [b], ascending, null_before, [va], [vb])
    # two key columns, the nullable one behind a leading column without nulls; mixed directions and placements
    a = [_column("int8", T + 3, rng), _column(dtype, T + 3, rng)]
    b = [_column("int8", T - 3, rng), _column(dtype, T - 3, rng)]
    _check_merge(gx, a, b, [not ascending, ascending], [True, null_before], [None, rng.random(T + 3) >= 0.4], [None, rng.random(T - 3) >= 0.4])


def test_merge_of_unsorted_rows_is_still_a_permutation(gx, T):
    """an unsorted side gives an unspecified order, but every row exactly once and nothing outside [0, na + nb)"""
    _, Column, ops = gx
    rng = np.random.default_rng(5)
    for na in (T + 1, 0, 3 * T):
        a = np.sort(rng.integers(0, 1000, na)).astype(np.int64)
        b = rng.integers(0, 1000, 3 * T).astype(np.int64)           # not sorted
        got = ops.merge_order([Column.from_numpy(a)], [Column.from_numpy(b)]).to_numpy()
        assert np.array_equal(np.sort(got), np.arange(na + 3 * T, dtype=np.int32))
    # nullable keys take the position-by-search path: entries in range is all it promises for unsorted rows
    v = rng.random(3 * T) >= 0.5
    got = ops.merge_order([Column.from_numpy(np.sort(b), np.ones(3 * T, bool) & (np.arange(3 * T) > 5))], [Column.from_numpy(b, v)]).to_numpy()
    assert got.min() >= 0 and got.max() < 6 * T


# ------------------------------------------------------------------------------------------------ payloads, slices, several tables
def _check_columns(outs, cols, valids, order):
    """every output column against input[order]: values bit for bit wherever the row is valid, the validity bits, the null count"""
    for o, c, v in zip(outs, cols, valids):
        assert o.size == len(order) and o.dtype == c.dtype
        want_valid = np.ones(len(order), bool) if v is None else v[order]
        got_valid = o.valid_numpy()
        if want_valid.all():
            assert o.mask is None and o.null_count == 0          # no nulls in the output: no mask comes back
        else:
            assert got_valid is not None and np.array_equal(got_valid, want_valid)
            assert o.null_count == int((~want_valid).sum())
        assert o.to_numpy()[want_valid].tobytes() == c[order][want_valid].tobytes()


@pytest.mark.parametrize("ntables", [1, 2, 3, 5])
def test_merge_sorted_tables_with_payloads(gx, T, ntables):
    """k tables with empty ones in between; payload columns of width 1 / 2 / 4 / 8, nullable ones among them (one whose nulls all stay
    in a table that is empty here, so its mask must not come back); ties come out by (table index, row)"""
    _, Column, ops = gx
    rng = np.random.default_rng(ntables)
    sizes = {1: [T + 1], 2: [T - 1, 3 * T + 7], 3: [2 * T, 0, T + 1], 5: [0, T + 3, 0, 5, 2 * T - 1]}[ntables]
    dts = ["int16", "int8", "float32", "int64", "uint16", "float64"]      # column 0 is the key (few values: many ties)
    tables_np, tables_dev = [], []
    for t, n in enumerate(sizes):
        cols = [rng.integers(0, 6, n).astype(dts[0])] + [_column(d, n, rng, few=False) for d in dts[1:]]
        valids = [None, rng.random(n) >= 0.3, None, rng.random(n) >= 0.5, rng.random(n) >= 0.1, np.ones(n, bool)]
        cols, valids = _sort_table_by_key(cols, valids)
        tables_np.append((cols, valids))
        tables_dev.append(_upload(Column, cols, valids))
    outs = ops.merge_sorted(tables_dev, [0], ascending=False)
    all_cols = [np.concatenate([tb[0][k] for tb in tables_np]) for k in range(len(dts))]
    all_valids = [np.concatenate([tb[1][k] if tb[1][k] is not None else np.ones(len(tb[0][k]), bool) for tb in tables_np]) for k in range(len(dts))]
    order = orc.sorted_order_rows([all_cols[0]], None, False, True)
    _check_columns(outs, all_cols, all_valids, order)


def _sort_table_by_key(cols, valids):
    if len(cols[0]) == 0:
        return cols, valids
    o = orc.sorted_order_rows([cols[0]], None, False, True)
    return [c[o] for c in cols], [None if v is None else v[o] for v in valids]


def _ptr_array(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def test_sliced_inputs_with_a_nonzero_begin_bit(gx, T):
    """the C ABI on views into larger columns: data pointers moved to row `off`, bitmaps read from bit `off` on (37 and 3: not word
    aligned) -- merge map, two-source gather with its null count, and the bounds"""
    cudf_amd, Column, ops = gx
    L = cudf_amd._lib
    lib = L.lib
    from cudf_amd.column import stream_ptr
    import torch
    rng = np.random.default_rng(99)
    offs, ns = (37, 3), (T + 5, 2 * T - 7)
    sides = []
    for off, n in zip(offs, ns):
        k0, k1 = _column("int32", n, rng), _column("float64", n, rng)
        v0 = rng.random(n) >= 0.3
        (k0, k1), (v0, _) = _sort_table([k0, k1], [v0, None], [True, False], [False, True])
        pay, vp = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64), rng.random(n) >= 0.4
        pad = lambda x, fill: np.concatenate([fill(off).astype(x.dtype), x, fill(11).astype(x.dtype)])   # noqa: E731
        junk = lambda m: rng.integers(0, 100, m)                                                          # noqa: E731
        junkb = lambda m: rng.integers(0, 2, m)                                                           # noqa: E731
        dev = [Column.from_numpy(pad(k0, junk), pad(v0, junkb)), Column.from_numpy(pad(k1, junk)), Column.from_numpy(pad(pay, junk), pad(vp, junkb))]
        sides.append(dict(k0=k0, k1=k1, v0=v0, pay=pay, vp=vp, dev=dev, off=off, n=n))
    A, B = sides
    dts = (ctypes.c_int * 2)(L.INT32, L.FLOAT64)
    desc, nbf = (ctypes.c_int * 2)(0, 1), (ctypes.c_int * 2)(0, 1)

    def arrays(s):
        d = s["dev"]
        return (_ptr_array([d[0].data.data_ptr() + 4 * s["off"], d[1].data.data_ptr() + 8 * s["off"]]), _ptr_array([d[0].mask.data_ptr(), None]),
                (ctypes.c_int64 * 2)(s["off"], 0))

    ad, av, ab = arrays(A)
    bd, bv, bb = arrays(B)
    n = A["n"] + B["n"]
    gmap = Column.empty(np.int32, n)
    nbytes = ctypes.c_size_t(0)
    assert lib.gx_merge_order(2, dts, ad, av, ab, A["n"], bd, bv, bb, B["n"], desc, nbf, None, None, ctypes.byref(nbytes), None) == 0
    tmp = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
    L.check(lib.gx_merge_order(2, dts, ad, av, ab, A["n"], bd, bv, bb, B["n"], desc, nbf, gmap.data_ptr, ctypes.c_void_p(tmp.data_ptr()),
                               ctypes.byref(nbytes), stream_ptr()), "gx_merge_order")
    want = _expected_map([A["k0"], A["k1"]], [A["v0"], None], [B["k0"], B["k1"]], [B["v0"], None], [True, False], [False, True])
    assert gmap.to_numpy().tobytes() == want.tobytes()
    # the payload through gx_gather2, both sides sliced
    out = Column.empty(np.int64, n, nullable=True)
    nulls = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    L.check(lib.gx_gather2(8, ctypes.c_void_p(A["dev"][2].data.data_ptr() + 8 * A["off"]), A["dev"][2].mask_ptr, A["off"], A["n"],
                           ctypes.c_void_p(B["dev"][2].data.data_ptr() + 8 * B["off"]), B["dev"][2].mask_ptr, B["off"], B["n"], gmap.data_ptr, n,
                           out.data_ptr, out.mask_ptr, ctypes.c_void_p(nulls.data_ptr()), stream_ptr()), "gx_gather2")
    pay, vp = np.concatenate([A["pay"], B["pay"]])[want], np.concatenate([A["vp"], B["vp"]])[want]
    assert np.array_equal(out.valid_numpy(), vp) and int(nulls.item()) == int((~vp).sum())
    assert out.to_numpy()[vp].tobytes() == pay[vp].tobytes()
    # bounds of B's rows in A, both sliced
    for upper in (0, 1):
        res = Column.empty(np.int32, B["n"])
        L.check(lib.gx_search_bounds(2, dts, ad, av, ab, A["n"], bd, bv, bb, B["n"], desc, nbf, upper, res.data_ptr, stream_ptr()), "gx_search_bounds")
        exp = _expected_bounds([A["k0"], A["k1"]], [A["v0"], None], [B["k0"], B["k1"]], [B["v0"], None], [True, False], [False, True], bool(upper))
        assert res.to_numpy().tobytes() == exp.tobytes()


@pytest.mark.parametrize("width", [1, 2, 4, 8])
def test_gather2_widths_and_one_sided_bitmaps(gx, T, width):
    """a bitmap on one side only: the other side counts as all valid; the null count is written on the device"""
    cudf_amd, Column, ops = gx
    L = cudf_amd._lib
    from cudf_amd.column import stream_ptr
    import torch
    rng = np.random.default_rng(width)
    dt = {1: np.int8, 2: np.uint16, 4: np.float32, 8: np.int64}[width]
    na, nb = T + 7, 2 * T - 9
    a, b = _column(dt, na, rng, few=False), _column(dt, nb, rng, few=False)
    vb = rng.random(nb) >= 0.25
    gmap = rng.permutation(na + nb).astype(np.int32)
    ca, cb, cm = Column.from_numpy(a), Column.from_numpy(b, vb), Column.from_numpy(gmap)
    for a_side, b_side, va_, vb_ in ((ca, cb, None, vb), (cb, ca, vb, None)):
        out = Column.empty(dt, na + nb, nullable=True)
        nulls = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        L.check(L.lib.gx_gather2(width, a_side.data_ptr, a_side.mask_ptr, 0, a_side.size, b_side.data_ptr, b_side.mask_ptr, 0, b_side.size,
                                 cm.data_ptr, na + nb, out.data_ptr, out.mask_ptr, ctypes.c_void_p(nulls.data_ptr()), stream_ptr()), "gx_gather2")
        x, y = a_side.to_numpy(), b_side.to_numpy()
        vals = np.concatenate([x, y])[gmap]
        valid = np.concatenate([np.ones(len(x), bool) if va_ is None else va_, np.ones(len(y), bool) if vb_ is None else vb_])[gmap]
        assert np.array_equal(out.valid_numpy(), valid) and int(nulls.item()) == int((~valid).sum())
        assert out.to_numpy()[valid].tobytes() == vals[valid].tobytes()
    # no bitmap anywhere: no out_valid needed, the count is 0
    out = Column.empty(dt, na + nb)
    nulls = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    L.check(L.lib.gx_gather2(width, ca.data_ptr, None, 0, na, cb.data_ptr, None, 0, nb, cm.data_ptr, na + nb, out.data_ptr, None,
                             ctypes.c_void_p(nulls.data_ptr()), stream_ptr()), "gx_gather2")
    assert out.to_numpy().tobytes() == np.concatenate([a, b])[gmap].tobytes() and int(nulls.item()) == 0


# ------------------------------------------------------------------------------------------------ search
def _expected_bounds(h_cols, h_valids, n_cols, n_valids, asc, nbf, upper):
    """lower: the oracle's stable order of needles || haystack -- a needle sits in front of every haystack row it ties with, so its
    position minus the needles in front of it is the number of haystack rows strictly below it.  upper: haystack || needles."""
    nh, nn = len(h_cols[0]), len(n_cols[0])
    if nn == 0:
        return np.zeros(0, np.int32)
    if upper:
        cols, valids = _concat(h_cols, h_valids, n_cols, n_valids)
        is_needle = lambda r: r >= nh      # noqa: E731
        needle_of = lambda r: r - nh       # noqa: E731
    else:
        cols, valids = _concat(n_cols, n_valids, h_cols, h_valids)
        is_needle = lambda r: r < nn       # noqa: E731
        needle_of = lambda r: r            # noqa: E731
    order = orc.sorted_order_rows(cols, valids, asc, nbf).astype(np.int64)
    nd = is_needle(order)
    before = np.cumsum(nd) - nd            # needles in front of each sorted position
    out = np.empty(nn, np.int32)
    pos = np.flatnonzero(nd)
    out[needle_of(order[pos])] = (pos - before[pos]).astype(np.int32)
    return out


def _check_bounds(gx, h_cols, n_cols, asc=True, nbf=True, h_valids=None, n_valids=None):
    _, Column, ops = gx
    k = len(h_cols)
    h_valids = h_valids or [None] * k
    n_valids = n_valids or [None] * k
    asc, nbf = _per(asc, k), _per(nbf, k)
    h_cols, h_valids = _sort_table(h_cols, h_valids, asc, nbf)
    hay, needles = _upload(Column, h_cols, h_valids), _upload(Column, n_cols, n_valids)
    for upper, fn in ((False, ops.lower_bound), (True, ops.upper_bound)):
        got = fn(hay, needles, asc, nbf)
        assert got.mask is None and got.dtype == np.int32
        want = _expected_bounds(h_cols, h_valids, n_cols, n_valids, asc, nbf, upper)
        assert got.to_numpy().tobytes() == want.tobytes(), ("upper" if upper else "lower")


@pytest.mark.parametrize("nhay", ["0", "1", "T", "2^20+3"])
def test_bounds_one_key_column(gx, T, nhay):
    """needles below, above and inside the haystack's range, equal to runs of duplicates, and none at all"""
    nh = {"0": 0, "1": 1, "T": T, "2^20+3": 2**20 + 3}[nhay]
    rng = np.random.default_rng(nh % 1000)
    hay = rng.integers(0, max(nh // 8, 4), nh).astype(np.int64) * 3          # runs of about 8 duplicates, gaps between the values
    needles = np.concatenate([np.array([-2**63, -5, -1, 2**63 - 1, 3 * max(nh // 8, 4) + 7], np.int64), rng.integers(-3, 3 * max(nh // 8, 4) + 3, 5000),
                              hay[rng.integers(0, nh, 3000)] if nh else np.zeros(0, np.int64)]).astype(np.int64)
    for asc in (True, False):
        _check_bounds(gx, [hay], [needles], asc)
    _check_bounds(gx, [hay], [np.zeros(0, np.int64)])


@pytest.mark.parametrize("dtype", DTYPES)
def test_bounds_for_every_dtype_with_null_and_nan_needles(gx, T, dtype):
    rng = np.random.default_rng(DTYPES.index(dtype) + 100)
    hay, needles = _column(dtype, T + 11, rng), _column(dtype, 3000, rng)
    for asc in (True, False):
        _check_bounds(gx, [hay], [needles], asc)
        for nbf in (True, False):
            _check_bounds(gx, [hay], [needles], asc, nbf, [rng.random(len(hay)) >= 0.2], [rng.random(len(needles)) >= 0.2])
            _check_bounds(gx, [hay], [needles], asc, nbf, None, [rng.random(len(needles)) >= 0.5])      # null needles, no null in the haystack


def test_bounds_with_several_key_columns(gx, T):
    rng = np.random.default_rng(3)
    dts, asc, nbf = ["int8", "float32", "uint64"], [False, True, False], [True, False, False]
    hay = [_column(d, 2 * T + 1, rng) for d in dts]
    needles = [_column(d, 4000, rng) for d in dts]
    _check_bounds(gx, hay, needles, asc, nbf)
    _check_bounds(gx, hay, needles, asc, nbf, [None, rng.random(2 * T + 1) >= 0.3, None], [rng.random(4000) >= 0.3, None, rng.random(4000) >= 0.1])
    wide = [DTYPES[k % len(DTYPES)] for k in range(32)]
    _check_bounds(gx, [(rng.integers(0, 2, T + 1)).astype(d) for d in wide], [(rng.integers(0, 2, 999)).astype(d) for d in wide],
                  [bool(k % 2) for k in range(32)])


def test_dataframe_searchsorted(gx, T):
    cudf_amd, Column, ops = gx
    rng = np.random.default_rng(8)
    a = np.sort(rng.integers(0, 500, T + 3)).astype(np.int64)
    v = rng.integers(-10, 510, 1000).astype(np.int64)
    df = cudf_amd.DataFrame({"a": a})
    for side in ("left", "right"):
        assert np.array_equal(df.searchsorted(v, side=side).to_numpy(), np.searchsorted(a, v, side=side))
        assert np.array_equal(df.searchsorted(cudf_amd.DataFrame({"a": v}), side=side).to_numpy(), np.searchsorted(a, v, side=side))
    # two columns, the second with nulls, descending / ascending, nulls first: against the oracle
    k0, k1, v1 = _column("int16", T, rng), _column("float64", T, rng), rng.random(T) >= 0.3
    for na_position, asc in (("first", [False, True]), ("last", [True, True]), ("last", [True, False])):
        nbf = [x ^ (na_position == "last") for x in asc]
        (s0, s1), (_, sv1) = _sort_table([k0, k1], [None, v1], asc, nbf)
        df = cudf_amd.DataFrame({"x": Column.from_numpy(s0), "y": Column.from_numpy(s1, sv1)})
        n0, n1, nv1 = _column("int16", 500, rng), _column("float64", 500, rng), rng.random(500) >= 0.3
        for side in ("left", "right"):
            got = df.searchsorted({"x": n0, "y": Column.from_numpy(n1, nv1)}, side=side, ascending=asc, na_position=na_position).to_numpy()
            want = _expected_bounds([s0, s1], [None, sv1], [n0, n1], [None, nv1], asc, nbf, side == "right")
            assert got.tobytes() == want.tobytes()
    with pytest.raises(ValueError):
        df.searchsorted({"x": n0}, side="left")


# ------------------------------------------------------------------------------------------------ the C++ surface
def test_cpp_merge_and_search_cases():
    """tests/cpp/cudf_merge_tests: cudf::merge / lower_bound / upper_bound through libcudf.so on small literal vectors"""
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "cudf_merge_tests")], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "0 failed" in r.stdout and "[ OK ] merge of three tables: ties come out by table index" in r.stdout
