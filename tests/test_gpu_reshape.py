"""GPU: gx_reshape.hip through the C ABI (begin bits, guard words, misaligned sources), the Python surface and the C++ binary.
Expected values come from plain NumPy on the host: np.stack(..., axis=1).ravel(), ndarray.T, np.tile, np.repeat, slice assignment
and init + arange * step.  Values are compared bit for bit (they move as bits: NaN payloads and -0.0 survive); validity words in
full, zero bits behind the last row and the guard word behind the bitmap included; the null count; the bytes behind the last
output row."""
import ctypes
import itertools
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ["int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float32", "float64", "bool"]
INTS = ["int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64"]
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
    return int(lib.gx_reshape_tile_rows())


# ------------------------------------------------------------------------------------------------ host helpers
def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype.itemsize])


def assert_same(got, want, what="", valid=None):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    eq = bits_of(got) == bits_of(want)
    if valid is not None:
        eq = eq | ~valid
    if not eq.all():
        i = int(np.flatnonzero(~eq)[0])
        raise AssertionError(f"{what}: {int((~eq).sum())} rows differ, first at {i}: got {got[i]!r}, want {want[i]!r}")


def random_bits(rng, width, n):
    return rng.integers(0, 256, n * width, dtype=np.uint8).view(UINT[width])   # every bit pattern: NaN payloads, -0.0, extremes


def random_values(rng, dt, n):
    dt = np.dtype(dt)
    if dt == np.bool_:
        return rng.integers(0, 2, n).astype(np.bool_)
    return rng.integers(0, 256, n * dt.itemsize, dtype=np.uint8).view(dt)


def dev(a, lead=0):
    """device bytes of a, `lead` bytes into a fresh allocation (lead = one element: a misaligned source)"""
    import torch
    a = np.ascontiguousarray(a)
    raw = a.view(np.uint8).reshape(-1)
    t = torch.zeros(lead + max(raw.size, 16), dtype=torch.uint8)
    t[lead: lead + raw.size] = torch.from_numpy(raw.copy())
    return t.cuda()[lead:]


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

    def check(self, want, want_valid, what=""):
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
        got = raw[: n * self.itemsize].view(UINT[self.itemsize])
        assert_same(got, bits_of(want), what)     # every row, null rows included: the kernels move them too


def stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def interleave(lib, cols, valids=None, begin_bits=None, lead=0, with_valid=None, rng=None):
    """gx_interleave over host columns (uint arrays of one width); valids: per column a bool array or None"""
    rng = rng or np.random.default_rng(1)
    k, n, w = len(cols), len(cols[0]), cols[0].dtype.itemsize
    valids = valids or [None] * k
    begin_bits = begin_bits or [0] * k
    with_valid = any(v is not None for v in valids) if with_valid is None else with_valid
    d = [dev(c, lead) for c in cols]
    m = [bitmap(v, b, rng) for v, b in zip(valids, begin_bits)]
    out = Out(n * k, w, with_valid)
    ptrs = (ctypes.c_void_p * k)(*[t.data_ptr() for t in d])
    vptrs = (ctypes.c_void_p * k)(*[t.data_ptr() if t is not None else None for t in m])
    bb = (ctypes.c_int64 * k)(*begin_bits)
    args = (w, k, ptrs, vptrs, bb, n, p(out.data), p(out.valid), p(out.nulls) if with_valid else None)
    nb = ctypes.c_size_t(0)
    assert lib.gx_interleave(*args, None, ctypes.byref(nb), None) == 0
    tmp = dev(np.zeros(max(nb.value, 16), np.uint8))
    assert lib.gx_interleave(*args, p(tmp), ctypes.byref(nb), stream()) == 0
    want = np.stack(cols, axis=1).ravel() if n else np.zeros(0, cols[0].dtype)
    want_valid = None
    if with_valid:
        want_valid = np.stack([np.ones(n, bool) if v is None else v for v in valids], axis=1).ravel() if n else np.zeros(0, bool)
    out.check(want, want_valid, f"interleave w={w} k={k} n={n} bits={list(begin_bits)} lead={lead}")


def tile_of(lib, elem, ncols):
    r, c = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.gx_interleave_tile(elem, ncols, ctypes.byref(r), ctypes.byref(c)) == 0
    return r.value, c.value


# ------------------------------------------------------------------------------------------------ interleave
@pytest.mark.parametrize("width", WIDTHS)
def test_interleave_rows_and_columns(lib, width):
    """row counts around the word, the wave and the band x column counts of the band regime, against np.stack(..., axis=1).ravel();
    every third shape carries nulls in some columns"""
    rng = np.random.default_rng(width)
    case = 0
    for k in (1, 2, 3, 5, 8, 16, 17):
        R, C = tile_of(lib, width, k)
        assert C == k
        for n in (0, 1, 31, 32, 33, 63, 64, 65, R - 1, R, R + 1, 3 * R + 17):
            cols = [random_bits(rng, width, n) for _ in range(k)]
            valids = None
            if case % 3 == 0:
                valids = [rng.integers(0, 4, n) > 0 if j % 2 == 0 else None for j in range(k)]
            interleave(lib, cols, valids, rng=rng)
            case += 1


@pytest.mark.parametrize("width", WIDTHS)
def test_interleave_two_dimensional(lib, width):
    """the wide regime: column counts around the tile's column count x a few rows, nulls in the odd columns"""
    rng = np.random.default_rng(10 + width)
    R, C = tile_of(lib, width, 4096)
    assert C < 4096
    for k in (C - 1, C, C + 1, 2 * C + 3):
        for n in (1, 2, 33, 65, R + 1):
            cols = [random_bits(rng, width, n) for _ in range(k)]
            valids = [rng.integers(0, 3, n) > 0 if j % 2 else None for j in range(k)]
            interleave(lib, cols, valids, rng=rng)
    interleave(lib, [random_bits(rng, width, 3) for _ in range(300)], rng=rng)      # more than one descriptor batch


@pytest.mark.parametrize("dt", DTYPES)
def test_interleave_dtypes(gx, dt):
    _, Column, ops = gx
    rng = np.random.default_rng(3)
    cols = [random_values(rng, dt, 70) for _ in range(3)]
    valids = [rng.integers(0, 3, 70) > 0, None, rng.integers(0, 3, 70) > 0]
    out = ops.interleave_columns([Column.from_numpy(c, v) for c, v in zip(cols, valids)])
    want_valid = np.stack([np.ones(70, bool) if v is None else v for v in valids], axis=1).ravel()
    assert out.dtype == np.dtype(dt) and out.size == 210 and out.null_count == int((~want_valid).sum())
    assert_same(out.to_numpy(), np.stack(cols, axis=1).ravel(), dt)
    assert (out.valid_numpy() == want_valid).all()
    plain = ops.interleave_columns([Column.from_numpy(c) for c in cols])
    assert plain.mask is None and plain.null_count == 0


def test_interleave_nullability_mixes(lib):
    """every mix of nullable and plain columns among three; a bitmap is asked for in all of them"""
    rng = np.random.default_rng(4)
    n = 77
    for mix in itertools.product((False, True), repeat=3):
        cols = [random_bits(rng, 4, n) for _ in range(3)]
        valids = [rng.integers(0, 2, n) > 0 if nullable else None for nullable in mix]
        interleave(lib, cols, valids, with_valid=True, rng=rng)


def test_interleave_begin_bits(lib):
    """begin bits 0 / 1 / 31 / 33, independently per column"""
    rng = np.random.default_rng(5)
    n = 97
    for bits in itertools.product(BEGIN_BITS, repeat=3):
        cols = [random_bits(rng, 2, n) for _ in range(3)]
        valids = [rng.integers(0, 2, n) > 0 for _ in range(3)]
        interleave(lib, cols, valids, begin_bits=list(bits), rng=rng)


@pytest.mark.parametrize("width", WIDTHS)
def test_interleave_misaligned_sources(lib, width):
    """source pointers one element off a 16-byte boundary: the element-wise way in"""
    rng = np.random.default_rng(6)
    for k, n in ((2, 1000), (5, 333), (40, 70)):
        interleave(lib, [random_bits(rng, width, n) for _ in range(k)], [rng.integers(0, 2, n) > 0] + [None] * (k - 1), lead=width, rng=rng)


def test_interleave_big(lib):
    """2^22 + 4097 output rows = 3 columns x 1399467 rows of int64"""
    rng = np.random.default_rng(7)
    assert BIG % 3 == 0
    n = BIG // 3
    interleave(lib, [random_bits(rng, 8, n) for _ in range(3)], [None, rng.integers(0, 8, n) > 0, None], rng=rng)


# ------------------------------------------------------------------------------------------------ transpose
@pytest.mark.parametrize("dt,shape", [("int32", (5, 3)), ("float64", (40, 33)), ("int8", (1, 7)), ("uint16", (70, 1))])
def test_transpose_twice(gx, dt, shape):
    _, Column, ops = gx
    rng = np.random.default_rng(8)
    n, k = shape
    a = random_values(rng, dt, n * k).reshape(n, k)
    valid = rng.integers(0, 3, (n, k)) > 0
    cols = [Column.from_numpy(a[:, j].copy(), valid[:, j].copy()) for j in range(k)]
    t = ops.transpose(cols)
    assert len(t) == n and all(c.size == k and c.dtype == np.dtype(dt) for c in t)
    got = np.stack([c.to_numpy() for c in t], axis=0)       # result column i is row i of the input
    assert_same(got.T.copy(), a.T.copy(), "transpose")
    for i, c in enumerate(t):
        assert c.null_count == int((~valid[i]).sum())
        if c.null_count:
            assert (c.valid_numpy() == valid[i]).all()
        else:
            assert c.mask is None
    back = ops.transpose(t)
    assert len(back) == k
    for j, c in enumerate(back):
        assert_same(c.to_numpy(), a[:, j].copy(), "transpose twice")
        assert c.null_count == int((~valid[:, j]).sum())
        if c.null_count:
            assert (c.valid_numpy() == valid[:, j]).all()
    assert ops.transpose([]) == [] and ops.transpose([Column.from_numpy(np.zeros(0, dt))]) == []


# ------------------------------------------------------------------------------------------------ tile / repeat with a scalar count
def tile_repeat(lib, fn, model, what, width, n, count, valid, begin_bit, rng):
    a = random_bits(rng, width, n)
    out = Out(n * count, width, valid is not None)
    m, d = bitmap(valid, begin_bit, rng), dev(a)
    rc = fn(width, p(d), p(m), begin_bit, n, count, p(out.data), p(out.valid), p(out.nulls) if valid is not None else None, stream())
    assert rc == 0
    out.check(model(a, count), None if valid is None else model(valid, count), f"{what} w={width} n={n} count={count} bit={begin_bit}")


@pytest.mark.parametrize("width", WIDTHS)
def test_tile(lib, T, width):
    rng = np.random.default_rng(20 + width)
    for n in (1, 3, 31, 32, 33, 1000, T + 1):
        for i, count in enumerate((0, 1, 2, 7, 65)):
            bit = BEGIN_BITS[(i + n) % 4]
            tile_repeat(lib, lib.gx_tile, np.tile, "tile", width, n, count, rng.integers(0, 3, n) > 0, bit, rng)
            tile_repeat(lib, lib.gx_tile, np.tile, "tile", width, n, count, None, 0, rng)


def test_tile_wraps_inside_a_word(lib):
    """3 rows laid down 2^20 times: ten and two thirds wraps per validity word"""
    rng = np.random.default_rng(30)
    tile_repeat(lib, lib.gx_tile, np.tile, "tile", 4, 3, 2**20, np.array([True, False, True]), 33, rng)
    tile_repeat(lib, lib.gx_tile, np.tile, "tile", 1, 1, 5000, np.array([False]), 1, rng)


@pytest.mark.parametrize("width", WIDTHS)
def test_repeat_scalar_count(lib, T, width):
    rng = np.random.default_rng(40 + width)
    for n in (1, 31, 33, 100, T + 1):
        for i, count in enumerate((0, 1, 2, 3, 64, 65)):
            bit = BEGIN_BITS[(i + n) % 4]
            tile_repeat(lib, lib.gx_repeat_each, np.repeat, "repeat_each", width, n, count, rng.integers(0, 3, n) > 0, bit, rng)
            tile_repeat(lib, lib.gx_repeat_each, np.repeat, "repeat_each", width, n, count, None, 0, rng)


# ------------------------------------------------------------------------------------------------ repeat with a count column
def repeat_map(lib, counts):
    """gx_repeat_map through the ABI: the map, with a guard behind it"""
    import torch
    counts = np.asarray(counts, dtype=np.int64)
    n, total = len(counts), int(counts.sum())
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    out = torch.full((total + 16,), -5, dtype=torch.int32, device="cuda")
    nb = ctypes.c_size_t(99)
    off = dev(offsets)
    assert lib.gx_repeat_map(p(off), n, total, p(out), None, ctypes.byref(nb), None) == 0
    tmp = dev(np.zeros(max(nb.value, 16), np.uint8))
    assert lib.gx_repeat_map(p(off), n, total, p(out), p(tmp), ctypes.byref(nb), stream()) == 0
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert (got[total:] == -5).all(), "the map was written behind its end"
    want = np.repeat(np.arange(n, dtype=np.int32), counts)
    bad = np.flatnonzero(got[:total] != want)
    assert not len(bad), f"{len(bad)} map entries differ, first at {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"


@pytest.fixture(scope="module")
def count_patterns(T):
    rng = np.random.default_rng(50)
    heavy = rng.integers(0, 2, 3000)
    heavy[1500] = 2**22
    ends = rng.integers(0, 8, 5000)
    ends[0] = ends[-1] = 0
    return {
        "all zero": np.zeros(3 * T + 5, np.int64),
        "all one": np.ones(3 * T + 5, np.int64),
        "uniform 0..7": rng.integers(0, 8, 4 * T + 3),
        "a run of zero counts three tiles long": np.concatenate([[1], np.zeros(3 * T, np.int64), [1]]),
        "zero runs between full tiles": np.concatenate([[T], np.zeros(3 * T + 1, np.int64), [2 * T, 0, 0, 5]]),
        "one row holds 2^22": heavy,
        "first and last row zero": ends,
        "one row": np.array([5]),
        "one row, many tiles": np.array([0, 0, 3 * T + 1, 0]),
    }


@pytest.mark.parametrize("name", ["all zero", "all one", "uniform 0..7", "a run of zero counts three tiles long",
                                  "zero runs between full tiles", "one row holds 2^22", "first and last row zero", "one row",
                                  "one row, many tiles"])
def test_repeat_map(lib, count_patterns, name):
    repeat_map(lib, count_patterns[name])


@pytest.mark.parametrize("name", ["uniform 0..7", "a run of zero counts three tiles long", "one row holds 2^22", "first and last row zero",
                                  "all zero"])
def test_repeat_count_column(gx, count_patterns, name):
    _, Column, ops = gx
    counts = count_patterns[name]
    rng = np.random.default_rng(51)
    n = len(counts)
    a = random_values(rng, "float64", n)
    valid = rng.integers(0, 3, n) > 0
    out = ops.repeat(Column.from_numpy(a, valid), Column.from_numpy(counts.astype(np.int64)))
    want_valid = np.repeat(valid, counts)
    assert out.size == int(counts.sum()) and out.null_count == int((~want_valid).sum())
    assert_same(out.to_numpy(), np.repeat(a, counts), name, want_valid)
    if out.null_count:
        assert (out.valid_numpy() == want_valid).all()


@pytest.mark.parametrize("cdt", INTS)
def test_repeat_count_dtypes_and_one_map_for_a_table(gx, cdt):
    """count columns of every integral dtype; three table columns of different widths, two with nulls, through one map"""
    _, Column, ops = gx
    rng = np.random.default_rng(52)
    n = 3000
    counts = rng.integers(0, 6, n)
    cols = [random_values(rng, dt, n) for dt in ("int8", "float32", "int64")]
    valids = [rng.integers(0, 3, n) > 0, None, rng.integers(0, 2, n) > 0]
    outs = ops.repeat([Column.from_numpy(c, v) for c, v in zip(cols, valids)], Column.from_numpy(counts.astype(cdt)))
    for c, v, o in zip(cols, valids, outs):
        wv = None if v is None else np.repeat(v, counts)
        assert o.dtype == c.dtype and o.size == int(counts.sum())
        assert_same(o.to_numpy(), np.repeat(c, counts), cdt, wv)
        if v is None:
            assert o.mask is None
        else:
            assert o.null_count == int((~wv).sum()) and (o.valid_numpy() == wv).all()


def test_repeat_total_of_two_to_the_31_overflows(gx):
    _, Column, ops = gx
    counts = Column.from_numpy(np.array([2**30, 0, 2**30], dtype=np.int64))
    with pytest.raises(OverflowError):
        ops.repeat(Column.from_numpy(np.arange(3, dtype=np.int8)), counts)
    ok = ops.repeat(Column.from_numpy(np.arange(3, dtype=np.int8)), Column.from_numpy(np.array([2, 0, 1], dtype=np.int64)))
    assert ok.to_numpy().tolist() == [0, 0, 2]


# ------------------------------------------------------------------------------------------------ sequence
def run_sequence(lib, gxmod, dt, n, init, step):
    dt = np.dtype(dt)
    out = Out(n, dt.itemsize, False)
    code = gxmod.column.gx_dtype(dt)
    init_dev = dev(np.array([init], dt))
    step_dev = dev(np.array([step], dt)) if step is not None else None
    rc = lib.gx_sequence(code, p(out.data), n, p(init_dev), p(step_dev), stream())
    assert rc == 0
    out.keep = (init_dev, step_dev)          # alive until the result has been read
    return out


@pytest.mark.parametrize("dt", INTS)
def test_sequence_integers(gx, lib, dt):
    """against (init + arange(n, uint64) * step) truncated to the width: wrap-around, a negative step, the default step"""
    dt = np.dtype(dt)
    top = np.iinfo(dt).max
    for n in (0, 1, 63, 64, 65, BIG):
        for init, step in ((top - 40, 3), (5, -7 if dt.kind == "i" else top - 6), (top, None)):
            i64 = np.array([init], dt).astype(np.int64 if dt.kind == "i" else np.uint64).view(np.uint64)[0]
            s64 = np.uint64(1) if step is None else np.array([step], dt).astype(np.int64 if dt.kind == "i" else np.uint64).view(np.uint64)[0]
            with np.errstate(over="ignore"):
                want = (i64 + np.arange(n, dtype=np.uint64) * s64).astype(UINT[dt.itemsize])
            run_sequence(lib, gx[0], dt, n, init, step).check(want, None, f"sequence {dt} n={n} init={init} step={step}")


def fused_model(dt, init, step, n):
    """init + i * step rounded ONCE (what a fused multiply-add gives), exactly, through rationals"""
    dt = np.dtype(dt)
    fi, fs = Fraction(float(dt.type(init))), Fraction(float(dt.type(step)))
    if dt == np.float64:
        return np.array([float(fi + i * fs) for i in range(n)], np.float64)
    out = np.empty(n, np.float32)
    for i in range(n):
        x = fi + i * fs
        d = np.float64(float(x))                     # correctly rounded to double, then to float: guard against double rounding
        f = np.float32(d)
        lo, hi = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
        out[i] = min((lo, f, hi), key=lambda c: (abs(Fraction(float(c)) - x), int(np.float32(c).view(np.uint32)) & 1))
    return out


@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_sequence_floats_round_twice(gx, lib, dt):
    """bit for bit against init + arange(n).astype(T) * step evaluated in T: the product is rounded, then the sum.  init = 1/3 and
    step = 0.1 give rows on which one rounding (a fused multiply-add) differs in the last bit: asserted here, on the host."""
    T_ = np.dtype(dt).type
    init, step = T_(1) / T_(3), T_(0.1)
    two = init + np.arange(4096).astype(T_) * step
    assert two.dtype == np.dtype(dt)
    one = fused_model(dt, init, step, 4096)
    assert (bits_of(two) != bits_of(one)).any(), "the fused and the two-rounding model agree on this input: the case is vacuous"
    for n in (0, 1, 63, 64, 65, BIG):
        want = init + np.arange(n).astype(T_) * step
        run_sequence(lib, gx[0], dt, n, init, step).check(want, None, f"sequence {dt} n={n}")
    want = init + np.arange(65).astype(T_) * T_(1)
    run_sequence(lib, gx[0], dt, 65, init, None).check(want, None, f"sequence {dt} default step")


# ------------------------------------------------------------------------------------------------ fill
@pytest.mark.parametrize("width", WIDTHS)
def test_fill_range(lib, width):
    """gx_fill_range against slice assignment over every range with ends in {0, 1, 31, 32, 33, n - 1, n}; rows outside the range and
    the bytes behind the column are kept"""
    import torch
    rng = np.random.default_rng(60 + width)
    n = 77
    ends = (0, 1, 31, 32, 33, n - 1, n)
    value = random_bits(rng, width, 1)
    vdev = dev(value)
    for b, e in itertools.product(ends, ends):
        if b > e:
            continue
        a = random_bits(rng, width, n)
        out = Out(n, width, False)
        out.data[: n * width] = dev(a)[: n * width]
        assert lib.gx_fill_range(width, p(out.data), b, e, p(vdev), stream()) == 0
        want = a.copy()
        want[b:e] = value[0]
        out.check(want, None, f"fill w={width} [{b}, {e})")
    big = torch.zeros(BIG * width + 64, dtype=torch.uint8, device="cuda")
    assert lib.gx_fill_range(width, p(big), 3, BIG - 5, p(vdev), stream()) == 0
    got = big.cpu().numpy()[: BIG * width].view(UINT[width])
    assert (got[3: BIG - 5] == value[0]).all() and not got[:3].any() and not got[BIG - 5:].any()


@pytest.mark.parametrize("dt", ["int8", "uint16", "float32", "int64", "bool"])
def test_fill(gx, dt):
    """ops.fill: valid and invalid scalars into nullable and plain columns"""
    _, Column, ops = gx
    rng = np.random.default_rng(61)
    n = 77
    ends = (0, 1, 31, 32, 33, n - 1, n)
    a = random_values(rng, dt, n)
    valid = rng.integers(0, 3, n) > 0
    value = np.array([1], dt)[0]
    for b, e in itertools.product(ends, ends):
        if b > e:
            continue
        for v in (valid, None):
            for scalar in (value, None):
                out = ops.fill(Column.from_numpy(a, v), b, e, scalar.item() if scalar is not None else None)
                want = a.copy()
                wv = np.ones(n, bool) if v is None else v.copy()
                if scalar is not None:
                    want[b:e] = scalar
                wv[b:e] = scalar is not None
                assert out.null_count == int((~wv).sum()), (b, e)
                assert_same(out.to_numpy(), want, f"fill [{b}, {e})", wv)
                if out.null_count:
                    assert (out.valid_numpy() == wv).all()
                else:
                    assert out.mask is None


# ------------------------------------------------------------------------------------------------ Python methods
def test_column_methods(gx):
    _, Column, ops = gx
    a = np.array([3, 1, 4, 1, 5], dtype=np.int32)
    valid = np.array([1, 0, 1, 1, 1], bool)
    c = Column.from_numpy(a, valid)
    r = c.repeat(3)
    assert r.to_numpy()[valid.repeat(3)].tolist() == a.repeat(3)[valid.repeat(3)].tolist() and r.null_count == 3
    counts = np.array([2, 3, 0, 1, 2], dtype=np.uint8)
    r = c.repeat(Column.from_numpy(counts))
    wv = valid.repeat(counts)
    assert r.size == 8 and r.null_count == 3 and (r.valid_numpy() == wv).all()
    assert r.to_numpy()[wv].tolist() == a.repeat(counts)[wv].tolist()
    for args in ((10,), (2, 11), (2, 11, 3), (11, 2, -2), (5, 5), (3, 2)):
        got = Column.arange(*args)
        want = np.arange(*args)
        assert got.dtype == want.dtype and got.to_numpy().tolist() == want.tolist(), args
    got = Column.arange(0, 70, 1, dtype=np.uint8).to_numpy()
    assert got.dtype == np.uint8 and got.tolist() == list(range(70))
    for dt in (np.float32, np.float64):
        start, stop, step = dt(1) / dt(3), dt(9), dt(0.1)
        got = Column.arange(start, stop, step, dtype=dt)
        n = int(np.ceil((stop - start) / step))
        want = start + np.arange(n).astype(dt) * step           # the two-rounding model
        assert got.size == n
        assert_same(got.to_numpy(), want, f"arange {dt}")


def test_dataframe_methods(gx):
    import pandas as pd
    cudf_amd, Column, ops = gx
    pdf = pd.DataFrame({"a": np.arange(6, dtype=np.int64), "b": np.arange(6, dtype=np.int64) * 10, "c": -np.arange(6, dtype=np.int64)})
    df = cudf_amd.DataFrame.from_pandas(pdf)
    got = df.repeat(2).to_pandas()
    pd.testing.assert_frame_equal(got, pdf.loc[pdf.index.repeat(2)].reset_index(drop=True))
    counts = np.array([0, 2, 1, 0, 3, 1])
    got = df.repeat(Column.from_numpy(counts)).to_pandas()
    pd.testing.assert_frame_equal(got, pdf.loc[pdf.index.repeat(counts)].reset_index(drop=True))
    inter = df.interleave_columns()
    assert inter.to_numpy().tolist() == pdf.to_numpy().ravel().tolist()
    t = df.T
    assert t.columns == [str(i) for i in range(6)] and len(t) == 3
    assert np.array_equal(t.to_pandas().to_numpy(), pdf.to_numpy().T)
    back = df.transpose().transpose()
    assert np.array_equal(back.to_pandas().to_numpy(), pdf.to_numpy())
    mixed = cudf_amd.DataFrame({"a": np.arange(3, dtype=np.int32), "b": np.arange(3, dtype=np.float64)})
    with pytest.raises(TypeError):
        mixed.T
    with pytest.raises(TypeError):
        mixed.interleave_columns()
    tiled = ops.tile([df["a"], df["b"]], 3)
    assert tiled[1].to_numpy().tolist() == np.tile(pdf["b"].to_numpy(), 3).tolist()


# ------------------------------------------------------------------------------------------------ the C++ surface
def test_cpp_reshape_binary():
    exe = os.path.join(ROOT, "tests", "cpp", "cudf_reshape_tests")
    assert os.path.exists(exe), "build the C++ tests first (make -C cudf_amd/cpp)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "0 failed" in r.stdout
