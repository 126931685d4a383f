"""GPU: cudf::scan / cudf::reduce at the edges of the kernels that run them today, PRODUCT, and uint16.

The constants are those of cudf_amd/csrc/gx_scan.hpp:
  * k_lookback_scan (integer SUM / PRODUCT, every MIN / MAX): tiles of LB_CHUNK = 16384 rows, LB_WIN = 16 predecessors read per
    look-back round -- 17 * 16384 + 1 rows is the first size at which a tile's first round cannot reach tile 0;
  * the three-launch scan (float SUM / PRODUCT): chunks of 4096 rows, their partials scanned in trips of 1024 -- a second trip
    needs more than 1024 * 4096 = 4 194 304 rows;
  * k_stream_reduce: 2048 rows per workgroup and trip, at most RED_MAX_BLOCKS = 2048 workgroups (more than 8 388 608 rows: the
    grid is capped and workgroups take further trips), then the scan of up to 2048 partials (second trip from 1025 partials).

References: numpy in the column / output type for integers (wrapping is the contract), the oracle's exact sums for float SUM
(1 ulp), a long-double cumprod for float PRODUCT with the bound written at _product_tolerance.

GPU time (MI355X): the 40 cases take 4.6 s together, 1.5 s of it the first import.  Per case: look-back scans (96 calls each)
0.04 - 0.19 s, three-launch chunk edges 0.01 s, the two 4 194 305-row scans 0.15 / 0.19 s, small reduces < 0.01 s, large reduces
0.03 - 0.46 s (float64 SUM at 8 392 705 rows: the exact CPU sum), integer PRODUCT 0.01 - 0.03 s, float PRODUCT 0.04 s.
Only the two 4 194 305-row scans and the two large reduce sizes exceed 700 001 rows.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cudf_oracle as orc

LB_CHUNK = 16384
SCAN_CHUNK = 4096
RED_TRIP = 2048        # SCAN_BT * 8 rows per workgroup and trip of k_stream_reduce
RED_MAX_BLOCKS = 2048
INTS = ["int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64"]


@pytest.fixture(scope="module")
def gx():
    import torch
    assert torch.cuda.is_available()
    import cudf_amd  # noqa: F401
    from cudf_amd import Column, ops
    return Column, ops


def _vals(dtype, n, rng):
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return (rng.random(n) * 2000 - 1000).astype(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)


def _ulps32(a, b):
    a, b = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return np.abs(np.where(a < 0, -(2**31) - a, a) - np.where(b < 0, -(2**31) - b, b))


def _assert_float_sum(got, want64, what):
    """1 ulp of the output type against the exact sum rounded to that type (a float32 output rounds the double result again)"""
    want = np.asarray(want64, np.float64).astype(got.dtype)
    d = orc.ulp_diff(got, want) if got.dtype == np.float64 else _ulps32(got, want)
    assert d.size == 0 or int(d.max()) <= 1, f"{what}: {int(d.max())} ulps at {int(np.argmax(d))}"


# ---------------------------------------------------------------------------------------------------------------------
# single-pass look-back scan
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,op", [("int32", "sum"), ("int64", "sum"), ("uint16", "sum"), ("uint16", "max"), ("int8", "min"),
                                      ("int8", "max"), ("float64", "min"), ("float64", "max")])
def test_lookback_scan_tile_edges(gx, dtype, op):
    Column, ops = gx
    rng = np.random.default_rng(31)
    for n in [LB_CHUNK - 1, LB_CHUNK, LB_CHUNK + 1, 2 * LB_CHUNK, 17 * LB_CHUNK + 1, 33 * LB_CHUNK + 5]:
        v = _vals(dtype, n, rng)
        if dtype == "float64":  # +-inf, +-0.0 and NaN: one value above +inf on every path (tests/test_gpu_float_extremes_nan.py)
            v[rng.integers(0, n, 64)] = rng.choice(np.array([np.inf, -np.inf, 0.0, -0.0]), 64)
            v[rng.integers(0, n, 3)] = np.nan  # anywhere: tile 0 and the rows before a tile edge included
            if n == 2 * LB_CHUNK:
                v[0] = np.nan                  # and row 0: the running maximum is NaN throughout
        tile = np.ones(n, bool)
        t0 = LB_CHUNK if n > 2 * LB_CHUNK - 1 else 0  # a whole tile of nulls: its aggregate is the identity
        tile[t0:t0 + LB_CHUNK] = False
        for mask in (None, rng.random(n) > 0.15, tile, np.zeros(n, bool)):
            col = Column.from_numpy(v, mask)
            for inclusive in (True, False):
                out = ops.scan(col, op, inclusive)
                ev, em = orc.scan(v, op, inclusive, mask)
                got = out.to_numpy()
                assert got.dtype == v.dtype
                if mask is None:
                    np.testing.assert_array_equal(got, ev, err_msg=f"{dtype} {op} n={n} inclusive={inclusive}")
                else:
                    np.testing.assert_array_equal(out.valid_numpy(), em)
                    np.testing.assert_array_equal(got[em], ev[em], err_msg=f"{dtype} {op} n={n} inclusive={inclusive} masked")


# ---------------------------------------------------------------------------------------------------------------------
# three-launch scan (float SUM)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_three_launch_scan_chunk_edges(gx, dtype):
    Column, ops = gx
    rng = np.random.default_rng(32)
    for n in [SCAN_CHUNK - 1, SCAN_CHUNK, SCAN_CHUNK + 1]:
        v = _vals(dtype, n, rng)
        for mask in (None, rng.random(n) > 0.15):
            x = v if mask is None else np.where(mask, v, 0).astype(v.dtype)
            prefix = orc.exact_prefix_sums(x)
            sel = np.ones(n, bool) if mask is None else mask
            for inclusive in (True, False):
                got = ops.scan(Column.from_numpy(v, mask), "sum", inclusive).to_numpy()
                want = prefix if inclusive else np.concatenate([[0.0], prefix[:-1]])
                _assert_float_sum(got[sel], want[sel], f"{dtype} n={n} inclusive={inclusive}")


def test_three_launch_scan_second_trip_of_partials(gx):
    """4 194 305 rows = 1025 chunks: the partials scan takes a second trip of 1024.  float64 SUM, inclusive.  The input is
    well-conditioned ON PURPOSE (positive multiples of 2^-40 in [0.5, 2.5): every prefix is below 2^24 and a multiple of 2^-40,
    i.e. fits the 64-bit mantissa of a long double), so the long-double cumsum is EXACT -- and a plain double cumsum is not
    (64 bits needed), so the low words of the double-double partials still have to cross the trip boundary intact."""
    Column, ops = gx
    assert np.finfo(np.longdouble).nmant >= 63
    n = 1024 * SCAN_CHUNK + 1
    rng = np.random.default_rng(33)
    v = 0.5 + rng.integers(0, 2**41, n).astype(np.float64) * 2.0 ** -40
    ref = np.cumsum(v.astype(np.longdouble))
    assert ref[-1] < 2.0 ** 24
    got = ops.scan(Column.from_numpy(v), "sum", True).to_numpy()
    _assert_float_sum(got, ref.astype(np.float64), "float64 sum n=4194305")
    assert (np.cumsum(v) != ref.astype(np.float64)).any()  # the plain double sum is not this reference


# ---------------------------------------------------------------------------------------------------------------------
# reduce
# ---------------------------------------------------------------------------------------------------------------------
def _reduce_out_dtype(dtype, op):
    k = np.dtype(dtype).kind
    if op in ("sum", "product"):
        return np.float64 if k == "f" else (np.uint64 if k == "u" else np.int64)
    return np.dtype(dtype).type


def _check_reduce(ops, Column, v, mask, op):
    out_dt = _reduce_out_dtype(v.dtype, op)
    got, ok = ops.reduce(Column.from_numpy(v, mask), op)
    exp, eok = orc.reduce(v, op, mask, out_dt)
    assert ok == eok
    if not ok:
        return
    if v.dtype.kind == "f" and op == "sum":
        _assert_float_sum(np.array([got]), np.array([exp]), f"{v.dtype} n={len(v)}")
    else:
        assert got == exp, (v.dtype, len(v), op, got, exp)


@pytest.mark.parametrize("dtype", INTS + ["float32", "float64"])
def test_reduce_trip_edges(gx, dtype):
    Column, ops = gx
    rng = np.random.default_rng(34)
    for n in [RED_TRIP - 1, RED_TRIP, RED_TRIP + 1]:
        v = _vals(dtype, n, rng)
        for mask in (None, rng.random(n) > 0.3):
            for op in ("sum", "min", "max"):
                _check_reduce(ops, Column, v, mask, op)


@pytest.mark.parametrize("n", [1025 * SCAN_CHUNK + 1, 2049 * SCAN_CHUNK + 1], ids=["1026_partials", "capped_grid_third_trip"])
@pytest.mark.parametrize("dtype,op", [("int64", "sum"), ("float64", "sum"), ("int8", "min"), ("uint16", "max")])
def test_reduce_partials_second_trip_and_grid_cap(gx, dtype, op, n):
    """4 198 401 rows = 1026 chunks: one workgroup per chunk, the scan of the partials takes a second trip.  8 392 705 rows = 2050
    chunks: the grid is capped at 2048 workgroups, which walk 2 x 2048 x 2048 rows in two trips and leave 4097 for a third.
    MIN / MAX: the only extreme is planted once as the last row and once as the first row of the last workgroup's last trip."""
    Column, ops = gx
    assert n in (4_194_305 + 4096, 8_392_705)
    rng = np.random.default_rng(35)
    v = _vals(dtype, n, rng)
    mask = rng.random(n) > 0.3
    if op == "sum":
        for m in (None, mask):
            _check_reduce(ops, Column, v, m, op)
        return
    info = np.iinfo(dtype)
    extreme = info.min if op == "min" else info.max
    v[v == extreme] = 0  # the planted row is the only one that holds the extreme
    nb = min(-(-n // SCAN_CHUNK), RED_MAX_BLOCKS)
    stride = nb * RED_TRIP
    first_of_last_trip = (nb - 1) * RED_TRIP + (n - 1 - (nb - 1) * RED_TRIP) // stride * stride
    assert (nb - 1) * RED_TRIP <= first_of_last_trip < n and first_of_last_trip + stride >= n
    for where in (n - 1, first_of_last_trip):
        w = v.copy()
        w[where] = extreme
        for m in (None, mask):
            if m is not None:
                m = m.copy()
                m[where] = True
            got, ok = ops.reduce(Column.from_numpy(w, m), op)
            assert ok and got == extreme, (dtype, op, n, where, got)
    _check_reduce(ops, Column, v, mask, op)  # and without the planted row


# ---------------------------------------------------------------------------------------------------------------------
# PRODUCT
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", INTS)
def test_integer_product_scan_and_reduce_wrap_exactly(gx, dtype):
    """ODD factors from the full range: odd values are units mod 2^k, so the product never collapses to 0 and every prefix
    carries information (a product of random full-range integers is 0 mod 2^64 after about 64 even factors)."""
    Column, ops = gx
    rng = np.random.default_rng(36)
    for n in [1, 63, LB_CHUNK + 1, 300_007]:
        v = _vals(dtype, n, rng) | np.dtype(dtype).type(1)
        for mask in (None, rng.random(n) > 0.15):
            col = Column.from_numpy(v, mask)
            for inclusive in (True, False):
                out = ops.scan(col, "product", inclusive)
                ev, em = orc.scan(v, "product", inclusive, mask)
                got = out.to_numpy()
                assert got.dtype == v.dtype
                assert np.all(ev[em] & 1 == 1)  # every expected prefix is odd: none has collapsed
                np.testing.assert_array_equal(got[em], ev[em], err_msg=f"{dtype} n={n} inclusive={inclusive}")
            out_dt = _reduce_out_dtype(dtype, "product")
            got, ok = ops.reduce(col, "product")
            exp, eok = orc.reduce(v, "product", mask, out_dt)
            assert ok and eok and np.asarray(got).dtype == np.dtype(out_dt) and got == exp, (dtype, n, got, exp)


def _product_tolerance(k, out_dtype):
    """relative bound for a product of k factors accumulated in double, in ANY association order:
    gamma_k = k u / (1 - k u) with u = 2^-53 (k - 1 roundings, (1 + u)^(k-1) - 1 <= gamma_k), plus one rounding of the output
    type (2^-53 for float64, 2^-24 for float32), plus the error of the long-double reference itself (k roundings of 2^-64)."""
    k = np.asarray(k, np.float64)
    u = 2.0 ** -53
    return k * u / (1 - k * u) + (2.0 ** -53 if np.dtype(out_dtype) == np.float64 else 2.0 ** -24) + k * 2.0 ** -64


def _unit_factors(dtype, n, rng):
    """1 +- U(0, 1e-3) and reciprocals: the running product is a random walk around 1, nothing under- or overflows"""
    f = 1.0 + rng.random(n) * 1e-3
    return np.where(rng.random(n) < 0.5, f, 1.0 / f).astype(dtype)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_float_product_scan_and_reduce(gx, dtype):
    Column, ops = gx
    assert np.finfo(np.longdouble).nmant >= 63
    rng = np.random.default_rng(37)
    for n in [SCAN_CHUNK + 1, 300_007]:
        v = _unit_factors(dtype, n, rng)
        for mask in (None, rng.random(n) > 0.15):
            x = (v if mask is None else np.where(mask, v, 1)).astype(np.longdouble)
            ref = np.cumprod(x)
            k = np.arange(1, n + 1)
            sel = np.ones(n, bool) if mask is None else mask
            col = Column.from_numpy(v, mask)
            for inclusive in (True, False):
                got = ops.scan(col, "product", inclusive).to_numpy()
                assert got.dtype == v.dtype
                r, kk = (ref, k) if inclusive else (np.concatenate([[1], ref[:-1]]), np.maximum(k - 1, 1))
                err = np.abs(got.astype(np.longdouble) - r) / np.abs(r)
                assert np.all(err[sel] <= _product_tolerance(kk, dtype)[sel]), (dtype, n, inclusive, float(err[sel].max()))
            got, ok = ops.reduce(col, "product")  # documented output type: float64
            assert ok and np.asarray(got).dtype == np.float64
            assert abs(np.longdouble(got) - ref[-1]) / abs(ref[-1]) <= _product_tolerance(n, np.float64)


def test_float_product_scan_second_trip_of_partials(gx):
    """the second operator of the three-launch path at 4 194 305 rows (1025 chunks): float32 PRODUCT, inclusive"""
    Column, ops = gx
    n = 1024 * SCAN_CHUNK + 1
    v = _unit_factors("float32", n, np.random.default_rng(38))
    ref = np.cumprod(v.astype(np.longdouble))
    got = ops.scan(Column.from_numpy(v), "product", True).to_numpy()
    err = np.abs(got.astype(np.longdouble) - ref) / np.abs(ref)
    assert np.all(err <= _product_tolerance(np.arange(1, n + 1), np.float32)), float(err.max())
