"""GPU: row filtering -- ops.apply_boolean_mask / drop_nulls / drop_nans / compare_scalar / selected_rows, DataFrame[mask] and
DataFrame.dropna (cudf_amd/csrc/gx_compact.hip under them).  Expected values are NumPy boolean indexing on the host copy of the
same inputs (pandas for the DataFrame methods); equality is bit-exact (tobytes()), floats included: NaN payloads and -0.0 survive.
Every case that is meant to drop something asserts that its mask keeps at least one row and drops at least one."""
import os
import subprocess

import numpy as np
import pytest

from tests import route_values as route

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64, np.float32, np.float64, np.bool_]
ROWS = [0, 1, 63, 64, 65, 4095, 4096, 4097, 1_000_003]


def _values(rng, dtype, n):
    """random BITS of the dtype: floats take every payload there is (quiet / signalling NaNs, infinities, -0.0, denormals)"""
    dt = np.dtype(dtype)
    if dt == np.bool_:
        return rng.integers(0, 2, n).astype(np.bool_)
    v = rng.integers(0, 256, n * dt.itemsize, dtype=np.uint8).view(dt)
    if dt.kind == "f" and n > 8:
        v[:4] = [np.nan, -0.0, np.inf, -np.inf]
    return v


def _mixed(mask):
    """a mask that keeps something and drops something"""
    assert mask.any() and not mask.all(), "the case must keep at least one row and drop at least one"
    return mask


def _check(out, values, valid, keep):
    """out == Column(values, valid)[keep], bit for bit; validity bits, null count and zero padding included"""
    exp = values[keep]
    assert out.size == len(exp) and out.dtype == values.dtype
    assert out.to_numpy().tobytes() == exp.tobytes()
    ev = None if valid is None else valid[keep]
    if ev is None or ev.all():
        assert out.mask is None and out.null_count == 0
        return
    assert out.mask is not None and out.null_count == int((~ev).sum())
    bits = np.unpackbits(out.mask.cpu().numpy().view(np.uint8), bitorder="little")
    assert np.array_equal(bits[: out.size].astype(bool), ev)
    assert not bits[out.size:].any(), "padding bits beyond the output length must be zero"


@pytest.fixture(scope="module")
def gx():
    import cudf_amd
    from cudf_amd import Column, ops
    return cudf_amd, Column, ops


# one input table per row count, built once: every dtype, every second column nullable
_RNG = np.random.default_rng(2024)
_TABLES = {}
for _n in ROWS:
    _cols = []
    for _k, _dt in enumerate(DTYPES):
        _cols.append((_values(_RNG, _dt, _n), (_RNG.random(_n) < 0.8) if (_k % 2 and _n) else None))
    _m = _RNG.random(_n) < 0.5
    if _n >= 2:
        _m[0], _m[1] = True, False
    _TABLES[_n] = (_cols, _m)


@pytest.mark.parametrize("n", ROWS)
def test_every_dtype_from_one_plan(gx, n):
    """10 numeric types + bool, 1 / 2 / 4 / 8-byte elements, as ONE table: one plan, eleven scatters"""
    _, Column, ops = gx
    cols, m = _TABLES[n]
    if n >= 2:
        _mixed(m)
    out = ops.apply_boolean_mask([Column.from_numpy(v, valid) for v, valid in cols], Column.from_numpy(m))
    assert len(out) == len(cols)
    for o, (v, valid) in zip(out, cols):
        _check(o, v, valid, m)


@pytest.mark.parametrize("kernel", [1, 2])
def test_both_scatter_kernels(gx, kernel):
    """gx_compact_set_kernel: 1 = the direct scatter, 2 = the LDS-staged one with 16-byte stores (columns without a bitmap): every
    width, chunk edges, output runs that start at every alignment inside a 16-byte lane"""
    cudf_amd, Column, ops = gx
    lib = cudf_amd._lib.lib
    lib.gx_compact_set_kernel(kernel)
    try:
        for n in (65, 4097, 1_000_003):
            cols, m = _TABLES[n]
            out = ops.apply_boolean_mask([Column.from_numpy(v) for v, _ in cols], Column.from_numpy(_mixed(m)))
            for o, (v, _) in zip(out, cols):
                _check(o, v, None, m)
        for name in ("1e-4", "0.999", "alternating", "runs of 10000"):
            m = _SEL_MASKS[name]
            out = ops.apply_boolean_mask([Column.from_numpy(v) for v, _ in _SEL_COLS], Column.from_numpy(m))
            for o, (v, _) in zip(out, _SEL_COLS):
                _check(o, v, None, m)
    finally:
        lib.gx_compact_set_kernel(0)


def _selectivity_masks(n):
    rng = np.random.default_rng(5)
    idx = np.arange(n)
    sparse = rng.random(n) < 1e-4
    sparse[n // 3] = True
    return {
        "none": np.zeros(n, dtype=bool),
        "all": np.ones(n, dtype=bool),
        "1e-4": sparse,
        "half": rng.random(n) < 0.5,
        "0.999": rng.random(n) < 0.999,
        "alternating": (idx % 2).astype(bool),
        "runs of 10000": ((idx // 10_000) % 2).astype(bool),      # whole 4096-row chunks empty, whole chunks full
    }


_SEL_N = 300_007
_SEL_RNG = np.random.default_rng(77)
_SEL_COLS = [(_values(_SEL_RNG, np.int64, _SEL_N), None), (_values(_SEL_RNG, np.int8, _SEL_N), _SEL_RNG.random(_SEL_N) < 0.6),
             (_values(_SEL_RNG, np.float32, _SEL_N), _SEL_RNG.random(_SEL_N) < 0.97)]
_SEL_MASKS = _selectivity_masks(_SEL_N)


@pytest.mark.parametrize("name", list(_SEL_MASKS))
def test_selectivities(gx, name):
    _, Column, ops = gx
    m = _SEL_MASKS[name]
    if name not in ("none", "all"):
        _mixed(m)
    out = ops.apply_boolean_mask([Column.from_numpy(v, valid) for v, valid in _SEL_COLS], Column.from_numpy(m))
    for o, (v, valid) in zip(out, _SEL_COLS):
        _check(o, v, valid, m)
    assert np.array_equal(ops.selected_rows(Column.from_numpy(m)).to_numpy(), np.flatnonzero(m).astype(np.int32))


def test_nullable_mask_and_bytes_other_than_0_and_1(gx):
    """a null mask element drops its row whatever its data byte holds; any non-zero byte is true"""
    _, Column, ops = gx
    rng = np.random.default_rng(9)
    n = 70_001
    raw = rng.integers(0, 256, n, dtype=np.uint8) * (rng.random(n) < 0.6)
    raw[:3] = [2, 255, 0]
    mvalid = rng.random(n) < 0.7
    mvalid[:3] = [True, False, True]
    keep = _mixed((raw != 0) & mvalid)
    assert ((raw > 1) & mvalid).any() and ((raw != 0) & ~mvalid).any()
    v = _values(rng, np.int32, n)
    valid = rng.random(n) < 0.5
    mask = Column.from_numpy(raw.view(np.bool_), mvalid)
    assert mask.to_numpy().view(np.uint8).max() > 1            # the bytes reached the device as they are
    out, = ops.apply_boolean_mask([Column.from_numpy(v, valid)], mask)
    _check(out, v, valid, keep)
    assert np.array_equal(ops.selected_rows(mask).to_numpy(), np.flatnonzero(keep).astype(np.int32))


def test_mask_at_an_unaligned_address(gx):
    """a mask whose bytes do not start on a 16-byte boundary takes the byte-per-lane selector: same result"""
    import torch
    _, Column, ops = gx
    rng = np.random.default_rng(10)
    n = 33_333
    m = _mixed(rng.random(n) < 0.4)
    v = _values(rng, np.uint16, n)
    for shift in (1, 5, 8):
        big = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
        big[shift: shift + n].copy_(torch.from_numpy(m.view(np.uint8)))
        mask = Column(big[shift:], np.bool_, n)
        assert mask.data.data_ptr() % 16 == shift
        out, = ops.apply_boolean_mask([Column.from_numpy(v)], mask)
        _check(out, v, None, m)


@pytest.mark.parametrize("nkeys", [1, 2, 3])
def test_drop_nulls(gx, nkeys):
    _, Column, ops = gx
    rng = np.random.default_rng(20 + nkeys)
    n = 50_003
    cols = [(_values(rng, dt, n), rng.random(n) < p) for dt, p in [(np.int32, 0.7), (np.float64, 0.5), (np.int8, 0.9)]]
    cols.append((_values(rng, np.int64, n), None))
    dev = [Column.from_numpy(v, valid) for v, valid in cols]
    keys = list(range(nkeys))
    nvalid = sum(cols[k][1].astype(int) for k in keys)
    for thr in (0, 1, nkeys, nkeys + 1):
        keep = nvalid >= thr
        if 0 < thr <= nkeys:
            _mixed(keep)
        out = ops.drop_nulls(dev, keys, thr)
        for o, (v, valid) in zip(out, cols):
            _check(o, v, valid, keep)
    out = ops.drop_nulls(dev, keys)                             # default threshold: every key valid
    for o, (v, valid) in zip(out, cols):
        _check(o, v, valid, _mixed(nvalid == nkeys))
    # keys without any null: the input comes back unchanged, whatever the threshold
    for thr in (None, 0, 5):
        out = ops.drop_nulls(dev, [3], thr)
        for o, (v, valid) in zip(out, cols):
            _check(o, v, valid, np.ones(n, dtype=bool))
    with pytest.raises(IndexError):
        ops.drop_nulls(dev, [4])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_drop_nans(gx, dtype):
    """quiet and signalling NaN payloads of both signs go, +-inf stay, a NULL element is not a NaN even when its bytes are one"""
    _, Column, ops = gx
    rng = np.random.default_rng(31)
    n = 40_001
    dt = np.dtype(dtype)
    u = np.uint32 if dt.itemsize == 4 else np.uint64
    exp_bits, frac_bits = (0x7F800000, 23) if dt.itemsize == 4 else (0x7FF0000000000000, 52)
    a = rng.standard_normal(n).astype(dt)
    kinds = rng.integers(0, 12, n)
    bits = a.view(u)
    quiet = exp_bits | (1 << (frac_bits - 1)) | 5
    signalling = exp_bits | 1                                   # quiet bit clear, payload non-zero
    sign = 1 << (dt.itemsize * 8 - 1)
    bits[kinds == 0] = quiet
    bits[kinds == 1] = signalling
    bits[kinds == 2] = quiet | sign
    bits[kinds == 3] = signalling | sign
    bits[kinds == 4] = exp_bits                                 # +inf
    bits[kinds == 5] = exp_bits | sign                          # -inf
    valid = rng.random(n) < 0.8
    assert (np.isnan(a) & ~valid).any() and np.isinf(a).any()
    b = rng.standard_normal(n).astype(np.float64)
    b[rng.random(n) < 0.3] = np.nan
    payload = _values(rng, np.int16, n)
    cols = [(a, valid), (b, None), (payload, None)]
    dev = [Column.from_numpy(v, vv) for v, vv in cols]
    a_ok = ~(np.isnan(a) & valid)                               # null -> counts as non-NaN
    b_ok = ~np.isnan(b)
    for keys, ok in (([0], a_ok.astype(int)), ([0, 1], a_ok.astype(int) + b_ok.astype(int))):
        for thr in (None, 0, 1, len(keys), len(keys) + 1):
            keep = ok >= (len(keys) if thr is None else thr)
            if thr is None or 0 < thr <= len(keys):
                _mixed(keep)
            out = ops.drop_nans(dev, keys, thr)
            for o, (v, vv) in zip(out, cols):
                _check(o, v, vv, keep)
    with pytest.raises(TypeError):
        ops.drop_nans(dev, [2])


_CMP_NP = {"eq": np.equal, "ne": np.not_equal, "lt": np.less, "le": np.less_equal, "gt": np.greater, "ge": np.greater_equal}


@pytest.mark.parametrize("dtype", [np.int32, np.int64, np.uint64, np.float64])
def test_compare_scalar_and_its_use_as_a_mask(gx, dtype):
    _, Column, ops = gx
    rng = np.random.default_rng(41)
    n = 30_011
    dt = np.dtype(dtype)
    if dt == np.uint64:
        v = rng.integers(2**63 - 50, 2**63 + 50, n, dtype=np.uint64)      # values on both sides of 2^63
        scalar = np.uint64(2**63 + 3)
        assert (v > np.uint64(2**63)).any()
    elif dt.kind == "f":
        v = np.round(rng.standard_normal(n), 1)
        v[rng.random(n) < 0.1] = np.nan
        v[:2] = [0.5, -0.0]
        scalar = 0.5
    else:
        v = rng.integers(-40, 40, n).astype(dt)
        scalar = -7
    valid = rng.random(n) < 0.9
    other = _values(rng, np.int64, n)
    for nullable in (False, True):
        col = Column.from_numpy(v, valid if nullable else None)
        for op, fn in _CMP_NP.items():
            with np.errstate(invalid="ignore"):
                exp = fn(v, dt.type(scalar))
            m = ops.compare_scalar(col, op, scalar)
            assert m.dtype == np.bool_ and m.size == n
            got = m.to_numpy()
            if nullable:
                assert m.null_count == col.null_count and np.array_equal(m.valid_numpy(), valid)
                exp = exp & valid                                    # a null row compares to nothing and is dropped as a mask
                assert np.array_equal(got[valid], exp[valid])
            else:
                assert m.mask is None and np.array_equal(got, exp)
            _mixed(exp)
            out, = ops.apply_boolean_mask([Column.from_numpy(other)], m)
            _check(out, other, None, exp)
    for sym, op in (("==", "eq"), ("!=", "ne"), ("<", "lt"), ("<=", "le"), (">", "gt"), (">=", "ge")):
        assert np.array_equal(ops.compare_scalar(col, sym, scalar).to_numpy(), ops.compare_scalar(col, op, scalar).to_numpy())
    with pytest.raises(ValueError):
        ops.compare_scalar(col, "<>", scalar)
    if dt.kind in "iu":
        with pytest.raises(OverflowError):
            ops.compare_scalar(col, "eq", -1 if dt.kind == "u" else 2**70)


@pytest.mark.parametrize("dtype", route.DTYPES)
def test_compare_scalar_dtype_routes(gx, dtype):
    """gx_compare_scalar picks the value type from the dtype: one wave and a tail row of the values that tell a wrong instantiation
    from the right one (tests/route_values.py) -- a signed column compared as unsigned puts its negative values above the scalar,
    a float compared as bits orders -0.0 and NaN."""
    _, Column, ops = gx
    v = route.route_values(dtype, seed=8)
    dt = v.dtype
    scalars = {"b": [True, False], "f": [0.0, -50.5]}.get(dt.kind) or [3, np.iinfo(dt).max // 2 + 1 if dt.kind == "u" else -3]
    col = Column.from_numpy(v)
    for scalar in scalars:
        for op, fn in _CMP_NP.items():
            with np.errstate(invalid="ignore"):
                exp = fn(v, dt.type(scalar))
            assert np.array_equal(ops.compare_scalar(col, op, scalar).to_numpy(), exp), (dtype, op, scalar)


def test_argument_errors(gx):
    _, Column, ops = gx
    a = Column.from_numpy(np.arange(10, dtype=np.int32))
    with pytest.raises(TypeError):
        ops.apply_boolean_mask([a], Column.from_numpy(np.ones(10, dtype=np.int8)))
    with pytest.raises(ValueError):
        ops.apply_boolean_mask([a], Column.from_numpy(np.ones(9, dtype=bool)))
    assert ops.apply_boolean_mask([], Column.from_numpy(np.ones(9, dtype=bool))) == []
    assert ops.selected_rows(Column.from_numpy(np.zeros(0, dtype=bool))).size == 0


def test_dataframe_mask_and_dropna_against_pandas(gx):
    import pandas as pd
    cudf_amd, Column, ops = gx
    DF = cudf_amd.DataFrame
    rng = np.random.default_rng(51)
    n = 60_007
    a = rng.standard_normal(n)
    a[rng.random(n) < 0.3] = np.nan
    b = rng.standard_normal(n).astype(np.float32)
    b[rng.random(n) < 0.5] = np.nan
    c = rng.integers(-5, 5, n)
    d = rng.standard_normal(n)
    d[rng.random(n) < 0.2] = np.nan
    pdf = pd.DataFrame({"a": a, "b": b, "c": c, "d": d})
    as_nulls = DF.from_pandas(pdf)                         # missing values as NULLS
    as_nans = DF({"a": a, "b": b, "c": c, "d": d})         # ... as NaN values
    mixed = DF({"a": as_nulls["a"], "b": b, "c": c, "d": as_nulls["d"]})
    assert as_nulls["a"].has_nulls() and not as_nans["a"].has_nulls()

    def same(got, exp):
        exp = exp.reset_index(drop=True)
        assert 0 < len(exp) < n
        pd.testing.assert_frame_equal(got.to_pandas(), exp, check_dtype=False)

    for gdf in (as_nulls, as_nans, mixed):
        same(gdf.dropna(), pdf.dropna())
        same(gdf.dropna(how="any", subset=["a", "b"]), pdf.dropna(how="any", subset=["a", "b"]))
        same(gdf.dropna(how="all", subset=["a", "b", "d"]), pdf.dropna(how="all", subset=["a", "b", "d"]))
        same(gdf.dropna(subset="d"), pdf.dropna(subset=["d"]))
        same(gdf.dropna(thresh=3), pdf.dropna(thresh=3))
        same(gdf.dropna(thresh=2, subset=["a", "b", "d"]), pdf.dropna(thresh=2, subset=["a", "b", "d"]))
        assert len(gdf.dropna(subset=["c"])) == n              # nothing missing in an integer column without nulls
        assert len(gdf.dropna(thresh=5)) == 0 and gdf.dropna(thresh=5).columns == list(pdf.columns)
        m = c > 1
        same(gdf[m], pdf[m])
        same(gdf[ops.compare_scalar(gdf["c"], ">", 1)], pdf[m])
        same(gdf[ops.compare_scalar(gdf["d"], "lt", 0.25)], pdf[pdf["d"] < 0.25])   # NaN / null rows compare false and go
    assert as_nans["c"] is as_nans._cols["c"]                  # a str key still returns the column
    with pytest.raises(TypeError):
        as_nans.dropna(how="any", thresh=1)
    with pytest.raises(ValueError):
        as_nans[np.ones(n - 1, dtype=bool)]
    with pytest.raises(KeyError):
        as_nans.dropna(subset=["zz"])


def test_2_pow_26_rows_of_int64(gx):
    """the count and an order-sensitive checksum (sum of value * (position + 1) mod 2^64), both sides in 64-bit wrap-around"""
    import torch
    _, Column, ops = gx
    n = 1 << 26
    col = ops.random_column(np.int64, n, seed=123)
    mask = ops.random_column(np.bool_, n, seed=456, lo=0, hi=2)
    hv, hm = col.to_numpy(), mask.to_numpy()
    _mixed(hm)
    assert 0.49 < hm.mean() < 0.51
    exp = hv[hm]
    with np.errstate(over="ignore"):
        want = int((exp.view(np.uint64) * np.arange(1, len(exp) + 1, dtype=np.uint64)).sum(dtype=np.uint64))
    out, = ops.apply_boolean_mask([col], mask)
    assert out.size == len(exp)
    t = out.data[: out.size * 8].view(torch.int64)
    got = int((t * torch.arange(1, out.size + 1, dtype=torch.int64, device="cuda")).sum().item()) % 2**64
    assert got == want
    assert out.data[:8].view(torch.int64).item() == exp[0] and t[-1].item() == exp[-1]


def test_cpp_surface_on_the_device():
    """tests/cpp/cudf_compaction_tests: the same small vectors through libcudf.so -- mixed widths from one plan, sliced views with a
    non-zero offset, the throwing cases, the empty-table cases"""
    import __graft_entry__ as ge
    ge.build()
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "cudf_compaction_tests")], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "0 failed" in r.stdout and "sliced views" in r.stdout
