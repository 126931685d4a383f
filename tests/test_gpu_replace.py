"""GPU: gx_replace.hip through the C ABI (begin bits, guard words), the Python surface and the C++ binary.  Expected values come
from plain NumPy on the host: the policy fill from np.maximum.accumulate over the valid row numbers, the others from np.where /
np.clip / a first-occurrence lookup.  Values are compared bit for bit on valid rows (NaN == NaN where a float result is compared as a
float); validity words in full, zero bits behind the last row and the guard word behind the bitmap included; the null count; the
bytes behind the last output row."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ["int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float32", "float64", "bool"]
FLOATS = ["float32", "float64"]
WIDTHS = (1, 2, 4, 8)
BEGIN_BITS = (0, 1, 31, 33)
BIG = 2**22 + 4097
GUARD = 0xA5A5A5A5
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


@pytest.fixture(scope="module")
def gx():
    import torch
    import cudf_amd
    from cudf_amd import Column, ops
    assert torch.cuda.is_available()
    return cudf_amd, Column, ops


@pytest.fixture(scope="module")
def lib(gx):
    return gx[0]._lib.lib


@pytest.fixture(scope="module")
def T(lib):
    return int(lib.gx_replace_tile_rows())


@pytest.fixture(scope="module")
def ROWS(T):
    return (0, 1, 31, 32, 33, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17)


# ------------------------------------------------------------------------------------------------ host helpers
def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype.itemsize])


def same(got, want):
    """bit for bit; NaN == NaN"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    eq = bits_of(got) == bits_of(want)
    if got.dtype.kind == "f":
        eq |= np.isnan(got) & np.isnan(want)
    return eq


def assert_same(got, want, what="", valid=None):
    eq = same(got, want)
    if valid is not None:
        eq = eq | ~valid
    if not eq.all():
        i = int(np.flatnonzero(~eq)[0])
        raise AssertionError(f"{what}: {int((~eq).sum())} rows differ, first at {i}: got {got[i]!r}, want {want[i]!r}")


def nearest_valid(valid, backward):
    """the model: the source row of every row (itself where it is valid), -1 where there is none"""
    n = len(valid)
    if n == 0:
        return np.zeros(0, np.int64)
    if not backward:
        return np.maximum.accumulate(np.where(valid, np.arange(n), -1))
    rev = np.maximum.accumulate(np.where(valid[::-1], np.arange(n), -1))
    return np.where(rev < 0, -1, n - 1 - rev)[::-1]


def random_values(rng, dt, n):
    dt = np.dtype(dt)
    if dt == np.bool_:
        return rng.integers(0, 2, n).astype(np.bool_)
    return rng.integers(0, 256, n * dt.itemsize, dtype=np.uint8).view(dt)       # every bit pattern: NaN payloads, -0.0, extremes


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    raw = a.view(np.uint8).reshape(-1)
    t = torch.zeros(max(raw.size, 16), dtype=torch.uint8)
    t[: raw.size] = torch.from_numpy(raw.copy())
    return t.cuda()


def p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def bitmap(valid, begin_bit, rng):
    """device words that hold `valid` from begin_bit on, random bits around it; None for valid None"""
    if valid is None:
        return None
    total = begin_bit + len(valid)
    bits = rng.integers(0, 2, ((total + 31) // 32 + 1) * 32).astype(np.uint8)
    bits[begin_bit:total] = valid
    return dev(np.packbits(bits, bitorder="little"))


class Out:
    """an output column: 0xCD bytes behind the last row, a guard word behind the last bitmap word, a poisoned null count"""

    def __init__(self, n, itemsize, with_valid=True):
        import torch
        self.n, self.itemsize = n, itemsize
        self.data = torch.full((n * itemsize + 64,), 0xCD, dtype=torch.uint8, device="cuda")
        self.valid = dev(np.full((n + 31) // 32 + 1, GUARD, np.uint32)) if with_valid else None
        self.nulls = torch.full((1,), -7, dtype=torch.int64, device="cuda")

    def check(self, dt, want, want_valid, what=""):
        import torch
        torch.cuda.synchronize()
        n, nw = self.n, (self.n + 31) // 32
        raw = self.data.cpu().numpy()
        assert (raw[n * self.itemsize:] == 0xCD).all(), f"{what}: bytes behind the last row were written"
        if want_valid is None:
            want_valid = np.ones(n, bool)
        if self.valid is not None:
            words = self.valid.cpu().numpy()[: 4 * (nw + 1)].view(np.uint32)
            assert words[nw] == GUARD, f"{what}: the word behind the bitmap was written"
            bits = np.unpackbits(words[:nw].view(np.uint8), bitorder="little").astype(bool)
            assert not bits[n:].any(), f"{what}: bits behind the last row are set"
            bad = np.flatnonzero(bits[:n] != want_valid)
            assert not len(bad), f"{what}: {len(bad)} validity bits differ, first at row {bad[0]}"
            assert int(self.nulls.item()) == (int((~want_valid).sum()) if n else -7), f"{what}: null count"
        assert_same(raw[: n * self.itemsize].view(dt), np.asarray(want, dtype=dt), what, want_valid)


# ------------------------------------------------------------------------------------------------ replace_nulls with a policy
def run_policy(lib, data, valid, backward, begin_bit=0, seed=0):
    rng = np.random.default_rng(seed)
    n, isz = len(data), data.dtype.itemsize
    d_in, d_valid = dev(data), bitmap(valid, begin_bit, rng)
    out = Out(n, isz)
    nb = ctypes.c_size_t(0)
    args = (isz, p(d_in), p(d_valid), begin_bit, n, int(backward), p(out.data), p(out.valid), p(out.nulls))
    assert lib.gx_replace_nulls_policy(*args, None, ctypes.byref(nb), None) == 0
    tmp = dev(np.zeros(max(nb.value, 16), np.uint8))
    assert lib.gx_replace_nulls_policy(*args, p(tmp), ctypes.byref(nb), None) == 0
    return out


def check_policy(lib, data, valid, backward, what, begin_bit=0):
    src = nearest_valid(valid, backward)
    want = data[np.maximum(src, 0)] if len(data) else data
    run_policy(lib, data, valid, backward, begin_bit).check(data.dtype, want, src >= 0, what)


@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("backward", [False, True])
def test_policy_fill_row_counts_and_widths(lib, ROWS, backward, width):
    rng = np.random.default_rng(10 * width + backward)
    for n in ROWS:
        data = random_values(rng, UINT[width], n)
        check_policy(lib, data, rng.random(n) < 0.5, backward, f"n={n}")


@pytest.mark.parametrize("backward", [False, True])
def test_policy_fill_structured_bitmaps(lib, T, backward):
    n = 3 * T + 17
    rng = np.random.default_rng(3)
    data = random_values(rng, np.uint64, n)
    rows = np.arange(n)

    def only(*r):
        v = np.zeros(n, bool)
        v[list(r)] = True
        return v

    def null_run(a, b):
        v = np.ones(n, bool)
        v[a:b] = False
        return v

    def words(pattern):
        return np.unpackbits(np.full((n + 31) // 32, pattern, np.uint32).view(np.uint8), bitorder="little")[:n].astype(bool)

    cases = {
        "all valid": np.ones(n, bool), "all null": np.zeros(n, bool), "row 0": only(0), "last row": only(n - 1),
        "row T-1": only(T - 1), "row T": only(T), "a null run of T rows on a tile": null_run(T, 2 * T),
        "a null run of 2T+5 rows from T-3": null_run(T - 3, 3 * T + 2), "first row of every tile": rows % T == 0,
        "last row of every tile": rows % T == T - 1, "alternating": rows % 2 == 0, "words 0x80000000": words(0x80000000),
        "words 0x00000001": words(0x00000001),
    }
    for what, valid in cases.items():
        check_policy(lib, data, valid, backward, what)


@pytest.mark.parametrize("backward", [False, True])
def test_policy_fill_begin_bits(lib, T, backward):
    rng = np.random.default_rng(4)
    for begin in BEGIN_BITS:
        for n in (65, 3 * T + 17):
            data = random_values(rng, np.uint32, n)
            check_policy(lib, data, rng.random(n) < 0.3, backward, f"begin={begin} n={n}", begin_bit=begin)


def test_policy_fill_long_carries(lib, T):
    """2^22 + 4097 rows at validity 0.001.  The carry pass has no loop -- two launches of fixed depth: an exclusive running max
    inside blocks of 1024 table entries, then over the blocks -- so the case is sized to need both levels: 1024 T + 4097 rows are
    more than 1024 tiles, and the null runs below cross the block boundary in either direction (PRECEDING: tiles 1000 .. 1024 are
    null, so tile 1024, the first entry of block 1, takes a row carried out of block 0; FOLLOWING mirrors the entries, there the
    null tiles 0 .. 2 sit at the end of the table)."""
    n = BIG
    assert n > 1024 * T
    rng = np.random.default_rng(5)
    data = random_values(rng, np.uint64, n)
    valid = rng.random(n) < 0.001
    valid[1000 * T: 1024 * T + T // 2] = False
    valid[: 2 * T + 5] = False
    for backward in (False, True):
        check_policy(lib, data, valid, backward, f"backward={backward}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_policy_fill_every_dtype_through_the_python_surface(gx, T, dtype):
    _, Column, ops = gx
    rng = np.random.default_rng(6)
    n = T + 1
    data = random_values(rng, dtype, n)
    valid = rng.random(n) < 0.4
    if np.dtype(dtype).kind == "f":
        data = data.copy()
        data[:14] = nan_specials(dtype)          # NaN payloads of both signs, -0.0, denormals: valid rows whose bits are carried
        valid[:14:2] = True
    col = Column.from_numpy(data, valid)
    for policy, backward in (("preceding", False), ("following", True)):
        src = nearest_valid(valid, backward)
        out = ops.replace_nulls(col, policy)
        ok = src >= 0
        assert out.null_count == int((~ok).sum())
        if out.null_count:
            assert np.array_equal(out.valid_numpy(), ok)
        else:
            assert out.mask is None
        got, want = out.to_numpy(), data[np.maximum(src, 0)]
        assert np.array_equal(bits_of(got)[ok], bits_of(want)[ok])      # carried as bits: payloads and -0.0 survive
    plain = Column.from_numpy(data)
    assert np.array_equal(bits_of(ops.replace_nulls(plain, "preceding").to_numpy()), bits_of(data))


# ------------------------------------------------------------------------------------------------ replace_nulls with a column / scalar
def run_replace(lib, fn, first, data, valid, repl, repl_valid, ibit, rbit, scalar_valid=None, with_valid=True, seed=0):
    rng = np.random.default_rng(seed)
    n, isz = len(data), data.dtype.itemsize
    is_scalar = scalar_valid is not None
    d_in, d_valid, d_repl, d_rvalid = dev(data), bitmap(valid, ibit, rng), dev(repl), bitmap(repl_valid, rbit, rng)
    d_sv = dev(np.array([scalar_valid], np.uint8)) if is_scalar and scalar_valid != "null-pointer" else None
    out = Out(n, isz, with_valid)
    rc = getattr(lib, fn)(first, p(d_in), p(d_valid), ibit, p(d_repl), p(d_rvalid), rbit, p(d_sv), int(is_scalar), n, p(out.data),
                          p(out.valid), p(out.nulls) if with_valid else None, None)
    assert rc == 0
    return out


@pytest.mark.parametrize("width", WIDTHS)
def test_replace_nulls_column_and_scalar(lib, ROWS, width):
    rng = np.random.default_rng(20 + width)
    dt = UINT[width]
    for n in ROWS:
        data, repl = random_values(rng, dt, n), random_values(rng, dt, n)
        valid, rvalid = rng.random(n) < 0.5, rng.random(n) < 0.5
        for ibit, rbit in ((0, 0), (1, 33), (31, 1)):
            want = np.where(valid, data, repl)
            run_replace(lib, "gx_replace_nulls", width, data, valid, repl, rvalid, ibit, rbit).check(dt, want, valid | rvalid, f"col n={n}")
        run_replace(lib, "gx_replace_nulls", width, data, valid, repl, None, 33, 0).check(dt, np.where(valid, data, repl), None, f"plain repl n={n}")
        # ... the same without an output bitmap: the caller knows there are no nulls
        run_replace(lib, "gx_replace_nulls", width, data, valid, repl, None, 1, 0, with_valid=False).check(dt, np.where(valid, data, repl), None)
        run_replace(lib, "gx_replace_nulls", width, data, None, repl, rvalid, 0, 31).check(dt, data, None, f"input without a bitmap n={n}")
        s = random_values(rng, dt, 1)
        for sv in (1, "null-pointer"):
            run_replace(lib, "gx_replace_nulls", width, data, valid, s, None, 31, 0, scalar_valid=sv).check(
                dt, np.where(valid, data, s[0]), None, f"valid scalar n={n}")
        run_replace(lib, "gx_replace_nulls", width, data, valid, s, None, 1, 0, scalar_valid=0).check(dt, data, valid, f"invalid scalar n={n}")


# ------------------------------------------------------------------------------------------------ replace_nans
def nan_specials(dtype):
    dt = np.dtype(dtype)
    u = UINT[dt.itemsize]
    if dt.itemsize == 4:
        pats = [0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFC12345, 0x7F800000, 0xFF800000, 0x80000000, 0, 1, 0x80000001,
                0x3F800000, 0xBF800000]
    else:
        pats = [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001, 0x7FFFFFFFFFFFFFFF, 0xFFF8000000012345,
                0x7FF0000000000000, 0xFFF0000000000000, 0x8000000000000000, 0, 1, 0x8000000000000001, 0x3FF0000000000000, 0xBFF0000000000000]
    return np.array(pats, dtype=u).view(dt)     # NaNs of both signs and several payloads, +-inf, +-0, denormals, +-1


@pytest.mark.parametrize("dtype", FLOATS)
def test_replace_nans(lib, gx, ROWS, dtype):
    L = gx[0]._lib
    code = L.FLOAT32 if dtype == "float32" else L.FLOAT64
    rng = np.random.default_rng(30)
    sp = nan_specials(dtype)
    for n in ROWS:
        data = sp[rng.integers(0, len(sp), n)]
        repl = (rng.random(n) * 100).astype(dtype)
        valid, rvalid = rng.random(n) < 0.6, rng.random(n) < 0.5          # null rows with NaN bits stay null
        take = valid & np.isnan(data)
        want = np.where(take, repl, data)
        run_replace(lib, "gx_replace_nans", code, data, valid, repl, rvalid, 33, 1).check(dtype, want, np.where(take, rvalid, valid), f"n={n}")
        run_replace(lib, "gx_replace_nans", code, data, valid, repl, None, 1, 0).check(dtype, want, valid, f"plain repl n={n}")
        take0 = np.isnan(data)
        run_replace(lib, "gx_replace_nans", code, data, None, repl, None, 0, 0, with_valid=False).check(dtype, np.where(take0, repl, data), None)
        s = np.array([7.5], dtype)
        run_replace(lib, "gx_replace_nans", code, data, valid, s, None, 31, 0, scalar_valid=1).check(dtype, np.where(take, s[0], data), valid, "scalar")
        run_replace(lib, "gx_replace_nans", code, data, valid, s, None, 0, 0, scalar_valid=0).check(dtype, data, valid & ~take, "invalid scalar")


# ------------------------------------------------------------------------------------------------ clamp
def run_clamp(lib, code, data, lo, hi, lo_r=None, hi_r=None, lo_valid=None, hi_valid=None):
    dt = data.dtype
    out = Out(len(data), dt.itemsize, with_valid=False)
    sc = [dev(np.array([v], dt)) if v is not None else None for v in (lo, lo_r, hi, hi_r)]
    vb = [dev(np.array([v], np.uint8)) if v is not None else None for v in (lo_valid, hi_valid)]
    d_in = dev(data)
    assert lib.gx_clamp(code, p(d_in), len(data), p(sc[0]), p(vb[0]), p(sc[1]), p(sc[2]), p(vb[1]), p(sc[3]), p(out.data), None) == 0
    return out


def clamp_model(x, lo, hi, lo_r, hi_r):
    """x < lo ? lo_replace : (x > hi ? hi_replace : x); None does not bound"""
    out = x.copy()
    below = x < lo if lo is not None else np.zeros(len(x), bool)
    above = (x > hi) & ~below if hi is not None else np.zeros(len(x), bool)
    if lo is not None:
        out[below] = lo if lo_r is None else lo_r
    if hi is not None:
        out[above] = hi if hi_r is None else hi_r
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_clamp(lib, gx, ROWS, dtype):
    L = gx[0]._lib
    dt = np.dtype(dtype)
    code = getattr(L, "BOOL8" if dtype == "bool" else dtype.upper())
    rng = np.random.default_rng(40)
    for n in ROWS[1:]:
        x = random_values(rng, dt, n)
        if dt.kind == "f":
            x = np.where(rng.random(n) < 0.5, (rng.standard_normal(n) * 100).astype(dt), x)     # finite values among every bit pattern
            lo, hi, ext = dt.type(-50.5), dt.type(60.25), (dt.type(-np.inf), dt.type(np.inf))
        elif dt.kind == "b":
            lo, hi, ext = np.False_, np.True_, (np.False_, np.True_)
        else:
            info = np.iinfo(dt)
            lo, hi = dt.type(info.min // 2 + 3), dt.type(info.max // 2 + 1)        # uint64: above 2^62; int64: near -2^62
            ext = (dt.type(info.min), dt.type(info.max))
            x[: min(n, 6)] = np.array([info.max, info.min, info.max - 1, info.min + 1, info.max // 2 + 1, info.max // 2 + 2], dt)[: min(n, 6)]
        with np.errstate(invalid="ignore"):
            want = np.clip(x, lo, hi)
        run_clamp(lib, code, x, lo, hi).check(dt, want, None, f"n={n}")
        run_clamp(lib, code, x, ext[0], ext[1]).check(dt, x if dt.kind != "f" else np.clip(x, *ext), None, "bounds at the extremes")
        run_clamp(lib, code, x, hi, lo).check(dt, clamp_model(x, hi, lo, None, None), None, "lo > hi")
        run_clamp(lib, code, x, lo, hi, lo_valid=0).check(dt, clamp_model(x, None, hi, None, None), None, "invalid lo")
        run_clamp(lib, code, x, lo, hi, hi_valid=0, lo_valid=1).check(dt, clamp_model(x, lo, None, None, None), None, "invalid hi")
        run_clamp(lib, code, x, None, hi).check(dt, clamp_model(x, None, hi, None, None), None, "no lo")
        run_clamp(lib, code, x, lo, hi, lo_r=ext[1], hi_r=ext[0]).check(dt, clamp_model(x, lo, hi, ext[1], ext[0]), None, "replacements")
    if dt.kind == "f":     # a NaN row passes through bit for bit
        x = nan_specials(dtype)
        out = run_clamp(lib, code, x, dt.type(-1), dt.type(1))
        got = out.data.cpu().numpy()[: x.nbytes].view(dt)
        assert np.array_equal(bits_of(got)[np.isnan(x)], bits_of(x)[np.isnan(x)])
    if dtype in ("uint64", "int64"):    # no comparison goes through double: neighbours of 2^63 / +-2^63 that a double cannot tell apart
        if dtype == "uint64":
            x = np.array([2**63 - 1, 2**63, 2**63 + 1, 2**64 - 1, 2**63 + 1025], dt)
            lo, hi = dt.type(2**63), dt.type(2**63 + 1024)
        else:
            x = np.array([2**63 - 1, 2**63 - 2, -2**63, -2**63 + 1, 2**63 - 1025], dt)
            lo, hi = dt.type(-2**63 + 1), dt.type(2**63 - 2)
        run_clamp(lib, code, x, lo, hi).check(dt, np.clip(x, lo, hi), None, "near 2^63")


def test_clamp_bool8_bytes_other_than_0_and_1_are_true(lib, gx):
    """gx_clamp reads is_bool from the dtype table: a BOOL8 byte of 2 or 255 is `true`, so [false, true] bounds nothing and every
    row keeps its byte, and [false, false] turns every non-zero byte into 0 (as UINT8 the byte 2 would pass hi = 1).  One wave and a
    tail row."""
    L = gx[0]._lib
    raw = np.random.default_rng(41).choice(np.array([0, 1, 2, 255], np.uint8), 65)
    raw[:4] = [2, 0, 255, 1]
    x = raw.view(np.bool_)
    run_clamp(lib, L.BOOL8, x, np.False_, np.True_).check(np.dtype(bool), x, None, "inside the bounds: the byte is kept")
    run_clamp(lib, L.BOOL8, x, np.False_, np.False_).check(np.dtype(bool), np.zeros(65, np.bool_), None, "above hi = false")
    run_clamp(lib, L.BOOL8, x, np.True_, np.True_).check(np.dtype(bool), np.where(raw == 0, 1, raw).astype(np.uint8).view(np.bool_), None,
                                                         "below lo = true")


# ------------------------------------------------------------------------------------------------ find_and_replace
def find_model(x, valid, old, new, new_valid):
    """out[i] = new[j] for the smallest j with x[i] == old[j] (the dtype's ==: NaN matches nothing, -0.0 == +0.0), valid rows only"""
    out, ok = x.copy(), valid.copy()
    keep = ~np.isnan(old) if old.dtype.kind == "f" else np.ones(len(old), bool)
    if not keep.any():
        return out, ok
    uniq, first = np.unique(old[keep], return_index=True)      # the first occurrence of every old value
    first = np.flatnonzero(keep)[first]
    pos = np.minimum(np.searchsorted(uniq, x), len(uniq) - 1)
    hit = valid & (uniq[pos] == x)
    out[hit], ok[hit] = new[first[pos[hit]]], new_valid[first[pos[hit]]]
    return out, ok


@pytest.mark.parametrize("dtype", DTYPES)
def test_find_and_replace(lib, gx, T, dtype):
    L = gx[0]._lib
    dt = np.dtype(dtype)
    code = getattr(L, "BOOL8" if dtype == "bool" else dtype.upper())
    chunk = int(lib.gx_find_and_replace_chunk())
    rng = np.random.default_rng(50)
    for m in (0, 1, 2, 64, chunk, chunk + 1, 3 * chunk + 5):
        n = 3 * T + 17 if m >= chunk else T + 65
        if dt.kind == "b" or dt.itemsize == 1:
            pool = np.arange(2 if dt.kind == "b" else 256).astype(dt)
        elif dt.kind == "f":
            pool = np.concatenate([np.arange(-40, 5000, dtype=np.float64) / 4, [np.nan, np.inf, -np.inf]]).astype(dt)
        else:
            pool = (np.arange(5000) * 3 - 40).astype(dt)
        x = pool[rng.integers(0, len(pool), n)]
        old = pool[rng.integers(0, len(pool), m)]
        new = random_values(rng, dt, m)
        if m >= 2:
            old[1] = old[0]                      # a duplicated old value: the first mapping wins
            x[:50] = old[0]
        if m > chunk:
            only_last = pool[-4] if dt.kind == "f" else pool[len(pool) // 2]
            old[old == only_last] = pool[0]
            old[m - 1] = only_last               # an old value whose only match lies in the last chunk
            x[50:90] = only_last
        if dt.kind == "f":
            x[100:110] = np.nan                  # NaN in the column and in the list matches nothing
            x[110:120] = -0.0                    # -0.0 in the column matches +0.0 in the list
            if m >= 64:
                old[5], old[7] = np.nan, 0.0
                old[(old == 0) & (np.arange(m) != 7)] = 1.0
                old[1] = old[0]
        valid = rng.random(n) < 0.8
        new_valid = rng.random(m) < 0.7
        for vi, nv, ibit, nbit in ((valid, new_valid, 33, 1), (None, None, 0, 0), (valid, None, 1, 0), (None, new_valid, 0, 31)):
            want, ok = find_model(x, np.ones(n, bool) if vi is None else vi, old, new, np.ones(m, bool) if nv is None else nv)
            out = Out(n, dt.itemsize, with_valid=vi is not None or nv is not None)
            r2 = np.random.default_rng(1)
            d = [dev(x), bitmap(vi, ibit, r2), dev(old), dev(new), bitmap(nv if m else None, nbit, r2)]
            rc = lib.gx_find_and_replace(code, p(d[0]), p(d[1]), ibit, n, p(d[2]), p(d[3]), p(d[4]), nbit, m, p(out.data), p(out.valid),
                                         p(out.nulls) if out.valid is not None else None, None)
            assert rc == 0
            out.check(dt, want, ok if out.valid is not None else None, f"m={m}")


# ------------------------------------------------------------------------------------------------ normalize_nans_and_zeros
@pytest.mark.parametrize("dtype", FLOATS)
def test_normalize_nans_and_zeros(lib, gx, ROWS, dtype):
    L = gx[0]._lib
    dt = np.dtype(dtype)
    code = L.FLOAT32 if dtype == "float32" else L.FLOAT64
    rng = np.random.default_rng(60)
    sp = nan_specials(dtype)
    qnan = np.array(np.nan, dt)
    assert bits_of(qnan.reshape(1))[0] == (0x7FC00000 if dt.itemsize == 4 else 0x7FF8000000000000)
    for n in ROWS:
        x = np.where(rng.random(n) < 0.5, sp[rng.integers(0, len(sp), n)], random_values(rng, dt, n))
        want = x.copy()
        want[np.isnan(x)] = qnan
        want[x == 0] = 0.0
        out = Out(n, dt.itemsize, with_valid=False)
        d_in = dev(x)
        assert lib.gx_normalize_nans_and_zeros(code, p(d_in), n, p(out.data), None) == 0
        import torch
        torch.cuda.synchronize()
        raw = out.data.cpu().numpy()
        assert (raw[n * dt.itemsize:] == 0xCD).all()
        assert np.array_equal(bits_of(raw[: n * dt.itemsize].view(dt)), bits_of(want)), f"n={n}"     # bit for bit, NaNs included
        assert lib.gx_normalize_nans_and_zeros(code, p(d_in), n, p(d_in), None) == 0                   # in place
        torch.cuda.synchronize()
        assert np.array_equal(bits_of(d_in.cpu().numpy()[: n * dt.itemsize].view(dt)), bits_of(want)), f"in place n={n}"


# ------------------------------------------------------------------------------------------------ Column / DataFrame against pandas
def test_column_and_dataframe_methods_match_pandas(gx):
    import pandas as pd
    cudf_amd, Column, ops = gx
    rng = np.random.default_rng(70)
    n = 10_007
    a = rng.integers(-5, 15, n).astype(np.float64)
    a[rng.random(n) < 0.3] = np.nan
    a[:3] = np.nan
    a[-3:] = np.nan
    x = rng.random(n) * 20 - 5
    x[rng.random(n) < 0.2] = np.nan
    iv = rng.integers(-5, 15, n)
    ivalid = rng.random(n) < 0.7
    k = rng.integers(0, 12, n).astype(np.int32)
    pdf = pd.DataFrame({"a": a, "x": x, "i": np.where(ivalid, iv.astype(np.float64), np.nan), "k": k})
    df = cudf_amd.DataFrame.from_pandas(pdf[["a", "x"]])
    df["i"] = Column.from_numpy(iv, ivalid)
    df["k"] = k
    assert df["i"].dtype == np.int64 and df["i"].null_count > 0

    def eq(got, want):
        pd.testing.assert_frame_equal(got.to_pandas(), want, check_dtype=False, check_exact=True)

    eq(df.fillna(0), pdf.fillna(0))
    assert df.fillna(7)["i"].dtype == np.int64 and df.fillna(7)["i"].mask is None
    eq(df.fillna({"a": 1, "i": -3}), pdf.fillna({"a": 1, "i": -3}))
    eq(df.fillna(method="ffill"), pdf.ffill())
    eq(df.ffill(), pdf.ffill())
    eq(df.bfill(), pdf.bfill())
    lead, trail = int(np.argmax(~np.isnan(a))), int(np.argmax(~np.isnan(a[::-1])))     # rows without a source stay null
    assert df.ffill()["a"].null_count == lead >= 3 and df.bfill()["a"].null_count == trail >= 3
    eq(df.clip(0, 10), pdf.clip(0, 10))
    eq(df.clip(lower=2), pdf.clip(lower=2))
    eq(df.clip(upper=3), pdf.clip(upper=3))
    eq(df.replace(1, 2), pdf.replace(1, 2))
    eq(df.replace([1, 2, 1], [20, 10, 99]), pdf.replace([1, 2], [20, 10]))
    s = df["i"]
    np.testing.assert_array_equal(s.fillna(4).to_numpy(), np.where(ivalid, iv, 4))
    np.testing.assert_array_equal(s.fillna(Column.from_numpy(k.astype(np.int64))).to_numpy(), np.where(ivalid, iv, k))
    got = s.replace([3], [None])
    assert np.array_equal(got.valid_numpy(), ivalid & (iv != 3)) and got.null_count == int((~(ivalid & (iv != 3))).sum())
    with pytest.raises(TypeError):
        df.fillna(0.5)                        # does not fit the integer columns: no upcast
    f = Column.from_numpy(np.array([1.0, np.nan, -0.0, np.nan]), np.array([True, True, True, False]))
    r = ops.replace_nans(f, 9.0)
    assert r.null_count == 1 and np.array_equal(r.to_numpy()[:3], [1.0, 9.0, -0.0])
    z = ops.normalize_nans_and_zeros(f)
    assert z.null_count == 1 and np.array_equal(bits_of(z.to_numpy())[:3], bits_of(np.array([1.0, np.nan, 0.0])))


# ------------------------------------------------------------------------------------------------ the C++ surface
def test_cpp_replace_tests_binary():
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "cudf_replace_tests")], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "14 run, 0 failed" in r.stdout
