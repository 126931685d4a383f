"""GPU: gx_quantile (select and sort paths), gx_quantile_lookup and the Python surface above them, against plain NumPy models
(tests/quantile_model.py).  Selection: the elements at the lower / higher rank must be, bit for bit, those of ops.sort of the valid
rows (an independent path: the keys-only radix sort).  Interpolation: the formulas of gx_quantile.hip evaluated in np.float64 and
compared bit for bit -- except that where the MODEL's linear / midpoint result is a NaN made by arithmetic (inf - inf, 0 * inf, a NaN
operand) only NaN-ness is compared: which payload and sign such a NaN carries differs between processors, not between formulas.
pandas computes a + (b - a) * frac, so against pandas the bound is derived: either formula makes at most three roundings of quantities
bounded by max(|a|, |b|), hence |got - pandas| <= 8 * 2^-53 * max(|a|, |b|); lower / higher / nearest are exact."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import quantile_model as qm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ["int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float32", "float64"]
BEGIN_BITS = (0, 1, 31, 33)
BIG = 2**22 + 4097
GUARD = 0xA5A5A5A5
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
QS = [0.0, 1e-9, 0.25, 0.5, 0.75, 1 - 1e-9, 1.0]
MODES = {"auto": 0, "select": 1, "sort": 2}
PATHS = {1: "select", 2: "select_direct", 3: "sort"}
INTERP = {name: code for code, name in enumerate(qm.INTERPS)}
assert INTERP == {"linear": 0, "lower": 1, "higher": 2, "midpoint": 3, "nearest": 4}


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
    return int(lib.gx_quantile_tile_rows())


# ------------------------------------------------------------------------------------------------ host helpers
def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype.itemsize])


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    raw = a.view(np.uint8).reshape(-1)
    t = torch.zeros(max(raw.size, 16), dtype=torch.uint8)
    t[: raw.size] = torch.from_numpy(raw.copy())
    return t.cuda()


def p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def bitmap_words(valid, begin_bit, rng):
    """host words that hold `valid` from begin_bit on, random bits in front, a guard word behind the last word a call may read"""
    total = begin_bit + len(valid)
    nw = (total + 31) // 32
    bits = rng.integers(0, 2, nw * 32).astype(np.uint8)
    bits[begin_bit:total] = valid
    bits[total:] = 1                                            # set bits behind the last row must not be counted
    return np.concatenate([np.packbits(bits, bitorder="little").view(np.uint32), np.array([GUARD], np.uint32)])


def gx_code(dt):
    from cudf_amd.column import gx_dtype
    return gx_dtype(np.dtype(dt))


def run_quantile(lib, vals, qs, interp, mode, valid=None, begin_bit=0, rng=None):
    """gx_quantile through the C ABI: {"f64", "elems" (nq, 2), "nvalid", "path"}"""
    import torch
    vals = np.ascontiguousarray(vals)
    n, nq = len(vals), len(qs)
    data = dev(vals)
    words = vm = None
    if valid is not None:
        words = bitmap_words(valid, begin_bit, rng or np.random.default_rng(0))
        vm = dev(words)
    f64 = torch.full((nq,), -777.0, dtype=torch.float64, device="cuda")
    elems = torch.full((2 * nq * vals.itemsize + 16,), 0xCD, dtype=torch.uint8, device="cuda")
    nvalid = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    path = ctypes.c_int(0)
    qarr = (ctypes.c_double * nq)(*qs)
    nb = ctypes.c_size_t(0)
    args = (gx_code(vals.dtype), p(data) if n else None, p(vm), begin_bit, n, qarr, nq, INTERP[interp], MODES[mode], p(f64), p(elems),
            p(nvalid), ctypes.byref(path))
    assert lib.gx_quantile(*args, None, ctypes.byref(nb), stream()) == 0
    tmp = torch.empty(nb.value + 16, dtype=torch.uint8, device="cuda")
    rc = lib.gx_quantile(*args, p(tmp), ctypes.byref(nb), stream())
    assert rc == 0, rc
    st = ctypes.c_int(-1)
    assert lib.gx_quantile_status(p(tmp), ctypes.byref(st), stream()) == 0 and st.value == 0, st.value
    torch.cuda.synchronize()
    if vm is not None:
        assert np.array_equal(vm.cpu().numpy()[: 4 * len(words)].view(np.uint32), words), "the bitmap (or its guard word) was written"
    raw = elems.cpu().numpy()
    assert (raw[2 * nq * vals.itemsize:] == 0xCD).all(), "bytes behind out_elems were written"
    return dict(f64=f64.cpu().numpy(), elems=raw[: 2 * nq * vals.itemsize].view(vals.dtype).reshape(nq, 2).copy(),
                nvalid=int(nvalid.item()), path=PATHS.get(path.value))


def assert_f64(got, want, interp, what=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    for j, (g, w) in enumerate(zip(got, want)):
        if np.isnan(w) and interp in ("linear", "midpoint"):
            assert np.isnan(g), f"{what}: q[{j}] = {g!r}, want a NaN"
        else:
            assert g.view(np.uint64) == w.view(np.uint64), f"{what}: q[{j}] = {g!r} ({g.view(np.uint64):#x}), want {w!r} ({w.view(np.uint64):#x})"


def assert_elems(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(bits_of(got), bits_of(want)), f"{what}: elements {got.tolist()} want {want.tolist()}"


_SORTED = {}


def sorted_by_the_sort(gx, vals, key=None):
    """the valid values as ops.sort orders them (cached per key): the reference for ties of +-0 and NaN payloads"""
    if key is not None and key in _SORTED:
        return _SORTED[key]
    _, Column, ops = gx
    s = ops.sort(Column.from_numpy(vals)).to_numpy() if len(vals) else vals.copy()
    assert np.array_equal(bits_of(s), bits_of(qm.stable_sorted(vals))), "ops.sort and the stable model disagree"
    if key is not None:
        _SORTED[key] = s
    return s


def expect_path(vals, mode):
    if mode == "sort":
        return "sort"
    w = qm.sortable_words(vals)
    return "select_direct" if int(w.max()) - int(w.min()) < qm.NBINS else "select"


def check_all_interps(gx, lib, vals, qs, mode, want_path, valid=None, begin_bit=0, key=None, rng=None, what=""):
    live = vals if valid is None else vals[valid]
    srt = sorted_by_the_sort(gx, live, key)
    for interp in qm.INTERPS:
        got = run_quantile(lib, vals, qs, interp, mode, valid, begin_bit, rng)
        w = f"{what} {mode} {interp}"
        assert got["nvalid"] == len(live), w
        assert got["path"] == want_path, (w, got["path"], want_path)
        if len(live) == 0:
            continue
        elems, f64 = qm.expected(srt, qs, interp)
        assert_elems(got["elems"], elems, w)
        assert_f64(got["f64"], f64, interp, w)


_UNIFORM = {}


def uniform_i64(n):
    if n not in _UNIFORM:
        _UNIFORM[n] = np.random.default_rng(n).integers(-2**63, 2**63 - 1, n, dtype=np.int64, endpoint=True)
    return _UNIFORM[n]


# ------------------------------------------------------------------------------------------------ paths
def row_counts(T):
    return [1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 37 * T + 5, BIG]


@pytest.mark.parametrize("mode", ["select", "sort"])
@pytest.mark.parametrize("which", range(12))
def test_paths(gx, lib, T, which, mode):
    n = row_counts(T)[which]
    vals = uniform_i64(n)
    check_all_interps(gx, lib, vals, QS, mode, expect_path(vals, mode), key=("uniform", n), what=f"n={n}")


def thresholds(lib):
    mr, sh = ctypes.c_int64(0), ctypes.c_double(0)
    lib.gx_quantile_get_thresholds(ctypes.byref(mr), ctypes.byref(sh))
    return mr.value, sh.value


def predict_auto(lib, vals, qs, valid=None):
    """the documented rule: SORT below min_rows; else the plan: SELECT_DIRECT for a span below 2048, SORT when the candidates
    exceed max_share * n, else SELECT -- with the candidate count computed here from the digit rule"""
    min_rows, share = thresholds(lib)
    n = len(vals)
    if n < min_rows:
        return "sort", None
    live = vals if valid is None else vals[valid]
    ranks = sorted({r for q in qs for r in qm.index(len(live), q)[:2]})
    plan = qm.select_plan(qm.sortable_words(live), ranks)
    if plan["direct"]:
        return "select_direct", 0
    return ("sort" if float(plan["c"]) > share * float(n) else "select"), plan["c"]


def test_auto_follows_the_documented_rule(gx, lib):
    vals = uniform_i64(BIG)
    qs = [0.1, 0.5, 0.9]
    want, c = predict_auto(lib, vals, qs)
    min_rows, share = thresholds(lib)
    if min_rows <= BIG and share >= 0.01:        # the shipped default enables the select path: three bins of 2048 are ~0.15 % of n
        assert want == "select" and 0 < c < 0.01 * BIG
    got = run_quantile(lib, vals, qs, "linear", "auto")
    assert got["path"] == want
    srt = sorted_by_the_sort(gx, vals, ("uniform", BIG))
    elems, f64 = qm.expected(srt, qs, "linear")
    assert_elems(got["elems"], elems)
    assert_f64(got["f64"], f64, "linear")
    small = uniform_i64(3 * 2048 + 1)             # below min_rows AUTO sorts without a look at the column
    assert run_quantile(lib, small, qs, "linear", "auto")["path"] == predict_auto(lib, small, qs)[0]


# ------------------------------------------------------------------------------------------------ value shapes
def shapes(T):
    n = 37 * T + 5
    rng = np.random.default_rng(5)
    out = {
        "all rows equal": np.full(n, -123456789012345, np.int64),
        "two distinct values": rng.choice(np.array([-5, 10**15], np.int64), n),
        "keys in [100, 10001)": rng.integers(100, 10001, n).astype(np.int64),
        "span below 2048": rng.integers(-1000, 1047, n).astype(np.int64),
        "sorted ramp": np.arange(n, dtype=np.int64) * 3 - 7,
        "reversed ramp": (np.arange(n, dtype=np.int64) * 3 - 7)[::-1].copy(),
        "1000 rows per distinct value": (rng.permutation(n) // 1000).astype(np.int64) * 1_000_003,
    }
    out["span below 2048"][:2] = (-1000, 1046)
    o = rng.integers(100, 10001, n).astype(np.int64)
    o[n // 3], o[2 * n // 3] = np.iinfo(np.int64).min, np.iinfo(np.int64).max
    out["one outlier at each extreme"] = o
    return out


SHAPES = ["all rows equal", "two distinct values", "keys in [100, 10001)", "span below 2048", "one outlier at each extreme",
          "sorted ramp", "reversed ramp", "1000 rows per distinct value"]


@pytest.mark.parametrize("name", SHAPES)
def test_value_shapes(gx, lib, T, name):
    vals = shapes(T)[name]
    for mode in ("select", "sort"):
        want = expect_path(vals, mode)
        if name in ("all rows equal", "span below 2048") and mode == "select":
            assert want == "select_direct"
        check_all_interps(gx, lib, vals, QS, mode, want, key=("shape", name), what=name)


def test_outliers_make_auto_take_the_sort_path(gx, lib, T):
    vals = shapes(T)["one outlier at each extreme"]
    d_min, d_share = thresholds(lib)
    try:
        lib.gx_quantile_set_thresholds(0, d_share)            # the rule past min_rows, at a test-sized column
        want, c = predict_auto(lib, vals, QS)
        assert want == "sort" and c >= len(vals) - 2           # every ordinary row shares the outliers' middle bin
        check_all_interps(gx, lib, vals, QS, "auto", "sort", key=("shape", "one outlier at each extreme"), what="outliers")
        ramp = shapes(T)["sorted ramp"]
        want, c = predict_auto(lib, ramp, [0.5])
        assert want == "select"
        check_all_interps(gx, lib, ramp, [0.5], "auto", "select", key=("shape", "sorted ramp"), what="ramp")
    finally:
        lib.gx_quantile_set_thresholds(-1, -1.0)
    assert thresholds(lib) == (d_min, d_share)


# ------------------------------------------------------------------------------------------------ dtypes
@pytest.mark.parametrize("dt", DTYPES)
def test_dtypes(gx, lib, T, dt):
    dt = np.dtype(dt)
    rng = np.random.default_rng(11)
    n = 5 * T + 3
    if dt.kind == "f":
        vals = rng.standard_normal(n).astype(dt) * dt.type(1e3)
    else:
        info = np.iinfo(dt)
        vals = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    for mode in ("select", "sort"):
        check_all_interps(gx, lib, vals, QS, mode, expect_path(vals, mode), key=("dtype", dt.name), what=dt.name)


@pytest.mark.parametrize("dt", ["int64", "uint64"])
def test_neighbours_of_two_to_the_63_and_beyond_two_to_the_53(gx, lib, dt):
    """out_elems is exact; out_f64 is the model's rounded doubles"""
    dt = np.dtype(dt)
    if dt == np.uint64:
        vals = np.array([2**63 - 2, 2**63 - 1, 2**63, 2**63 + 1, 2**63 + 2, 2**64 - 1, 2**53 + 1, 2**53 + 3, 0, 2**64 - 2], dtype=np.uint64)
    else:
        vals = np.array([2**63 - 1, 2**63 - 2, -2**63, -2**63 + 1, 2**53 + 1, -(2**53) - 1, 2**53 + 3, 0, 2**62 + 1, -(2**62) - 3], dtype=np.int64)
    vals = np.tile(vals, 7)[: 67]
    qs = [k / 66 for k in range(67)][:64]
    for mode in ("select", "sort"):
        check_all_interps(gx, lib, vals, qs, mode, expect_path(vals, mode), what=dt.name)
    got = run_quantile(lib, vals, [1.0], "lower", "select")
    assert int(got["elems"][0, 0]) == int(vals.max()) and got["f64"][0] == np.float64(vals.max())


def test_bool8_is_refused(lib):
    from cudf_amd import _lib as L
    nb = ctypes.c_size_t(0)
    q = (ctypes.c_double * 1)(0.5)
    assert lib.gx_quantile(L.BOOL8, None, None, 0, 10, q, 1, 0, 0, None, None, None, None, None, ctypes.byref(nb), None) == -2


# ------------------------------------------------------------------------------------------------ floats
def float_column(dt, n, rng):
    dt = np.dtype(dt)
    u = UINT[dt.itemsize]
    vals = (rng.standard_normal(n) * 4).astype(dt)
    tiny = np.finfo(dt).smallest_subnormal
    special = np.array([0.0, -0.0, np.inf, -np.inf, tiny, -tiny, tiny * 3, np.finfo(dt).max, -np.finfo(dt).max], dtype=dt)
    idx = rng.permutation(n)
    k = n // 10
    vals[idx[:k]] = special[rng.integers(0, len(special), k)]
    vals[idx[k: 2 * k]] = rng.choice(np.array([0.0, -0.0], dtype=dt), k)        # a long run of zeros of both signs
    quiet = {4: 0x7FC00000, 8: 0x7FF8000000000000}[dt.itemsize]
    sign = 1 << (8 * dt.itemsize - 1)
    payloads = np.array([quiet, quiet | 1, quiet | 0x1234, quiet | sign, quiet | sign | 77], dtype=u).view(dt)
    vals[idx[2 * k: 3 * k]] = payloads[rng.integers(0, len(payloads), k)]       # NaNs with several payloads and both signs
    return vals


@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_floats(gx, lib, T, dt):
    rng = np.random.default_rng(13)
    n = 9 * T + 11
    vals = float_column(dt, n, rng)
    nan_share = np.isnan(vals).mean()
    assert 0.05 < nan_share < 0.2
    qs = QS + [0.15, 0.2, 1 - nan_share, 1 - nan_share / 2, 0.95, 0.999]         # zeros' run, the edge of the NaN run, inside it
    for mode in ("select", "sort"):
        check_all_interps(gx, lib, vals, qs, mode, expect_path(vals, mode), key=("floats", dt), what=dt)
    # small: every rank of a column that is mostly ties
    small = float_column(dt, 60, np.random.default_rng(14))
    check_all_interps(gx, lib, small, [k / 59 for k in range(60)], "select", "select", what=f"{dt} small")
    zeros = np.random.default_rng(15).choice(np.array([0.0, -0.0], dtype=dt), 3 * T + 1)
    check_all_interps(gx, lib, zeros, QS, "select", "select_direct", what=f"{dt} zeros")


@pytest.mark.parametrize("dt", ["float32", "float64"])
def test_column_of_only_nan(gx, lib, T, dt):
    dt = np.dtype(dt)
    quiet = {4: 0x7FC00000, 8: 0x7FF8000000000000}[dt.itemsize]
    n = 2 * T + 5
    vals = (np.arange(n).astype(UINT[dt.itemsize]) % 5 + quiet).astype(UINT[dt.itemsize]).view(dt)
    for mode, want in (("select", "select_direct"), ("sort", "sort")):
        check_all_interps(gx, lib, vals, QS, mode, want, what=f"{dt.name} NaN")


# ------------------------------------------------------------------------------------------------ bitmaps
@pytest.mark.parametrize("share", [0.8, 0.001])
def test_bitmaps(gx, lib, T, share):
    rng = np.random.default_rng(17)
    n = 37 * T + 5
    vals = uniform_i64(n)
    valid = rng.random(n) < share
    assert valid.any()
    for begin_bit in BEGIN_BITS:
        for mode in ("select", "sort"):
            live = vals[valid]
            check_all_interps(gx, lib, vals, [0.0, 0.3, 0.5, 1.0], mode, expect_path(live, mode), valid, begin_bit, key=("bitmap", share),
                              rng=rng, what=f"validity {share} begin {begin_bit}")


def test_bitmap_edges(gx, lib, T):
    rng = np.random.default_rng(19)
    for n in (1, 31, 32, 33, 63, 64, 65, T + 1):
        vals = rng.integers(-50, 50, n).astype(np.int32)
        valid = rng.random(n) < 0.5
        valid[rng.integers(0, n)] = True
        for begin_bit in BEGIN_BITS:
            for mode in ("select", "sort"):
                check_all_interps(gx, lib, vals, [0.0, 0.5, 1.0], mode, expect_path(vals[valid], mode), valid, begin_bit, rng=rng,
                                  what=f"n={n} begin {begin_bit}")


def test_all_null(lib, T):
    n = 3 * T + 7
    vals = uniform_i64(n)
    valid = np.zeros(n, bool)
    for mode in ("select", "sort", "auto"):
        for begin_bit in (0, 33):
            assert run_quantile(lib, vals, [0.5], "linear", mode, valid, begin_bit)["nvalid"] == 0
    assert run_quantile(lib, vals[:0], [0.5], "linear", "auto")["nvalid"] == 0


# ------------------------------------------------------------------------------------------------ gx_quantile_lookup
def run_lookup(lib, vals, qs, interp, exact, offsets, valid=None, begin_bit=0, order=None, counts=None, rng=None):
    import torch
    vals = np.ascontiguousarray(vals)
    nseg, nq = len(offsets) - 1, len(qs)
    total = nseg * nq
    data = dev(vals)
    vm = dev(bitmap_words(valid, begin_bit, rng or np.random.default_rng(0))) if valid is not None else None
    od = dev(np.asarray(order, np.int32)) if order is not None else None
    cd = dev(np.asarray(counts, np.int32)) if counts is not None else None
    off = dev(np.asarray(offsets, np.int32))
    item = 8 if exact else vals.itemsize
    out = torch.full((total * item + 64,), 0xCD, dtype=torch.uint8, device="cuda")
    nw = (total + 31) // 32
    ov = dev(np.full(nw + 1, GUARD, np.uint32))
    nulls = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    qarr = (ctypes.c_double * nq)(*qs)
    rc = lib.gx_quantile_lookup(gx_code(vals.dtype), p(data), p(vm), begin_bit, p(od), nseg, p(off), p(cd), qarr, nq, INTERP[interp], int(exact),
                                p(out), p(ov), p(nulls), stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    raw = out.cpu().numpy()
    assert (raw[total * item:] == 0xCD).all(), "bytes behind the last result were written"
    words = ov.cpu().numpy()[: 4 * (nw + 1)].view(np.uint32)
    assert words[nw] == GUARD, "the word behind the result bitmap was written"
    bits = np.unpackbits(words[:nw].view(np.uint8), bitorder="little").astype(bool)
    assert not bits[total:].any()
    got = raw[: total * item].view(np.float64 if exact else vals.dtype)
    return got, bits[:total], int(nulls.item())


def lookup_model(vals, qs, interp, exact, offsets, valid=None, order=None, counts=None):
    nseg, nq = len(offsets) - 1, len(qs)
    out = np.zeros(nseg * nq, np.float64 if exact else vals.dtype)
    ok = np.zeros(nseg * nq, bool)
    for s in range(nseg):
        beg = offsets[s]
        cnt = counts[s] if counts is not None else offsets[s + 1] - beg
        if cnt == 0:
            continue
        for j, q in enumerate(qs):
            ix = qm.index(cnt, q)
            ra = order[beg + ix[0]] if order is not None else beg + ix[0]
            rb = order[beg + ix[1]] if order is not None else beg + ix[1]
            use_a = interp in ("linear", "midpoint", "lower") or (interp == "nearest" and ix[2] == ix[0])
            use_b = interp in ("linear", "midpoint", "higher") or (interp == "nearest" and ix[2] != ix[0])
            if valid is not None and ((use_a and not valid[ra]) or (use_b and not valid[rb])):
                continue
            ok[s * nq + j] = True
            r = qm.interpolate(interp, vals[ra], vals[rb], ix)
            if exact:
                out[s * nq + j] = r
            elif interp in ("linear", "midpoint"):
                out[s * nq + j] = np.float64(r).astype(vals.dtype)
            else:
                out[s * nq + j] = vals[ra] if use_a else vals[rb]
    return out, ok


def check_lookup(lib, vals, qs, exact, offsets, valid=None, begin_bit=0, order=None, counts=None, rng=None, what=""):
    for interp in qm.INTERPS:
        got, ok, nulls = run_lookup(lib, vals, qs, interp, exact, offsets, valid, begin_bit, order, counts, rng)
        want, want_ok = lookup_model(vals, qs, interp, exact, offsets, valid, order, counts)
        w = f"{what} {interp}"
        assert np.array_equal(ok, want_ok), w
        assert nulls == int((~want_ok).sum()), w
        assert np.array_equal(bits_of(got)[ok], bits_of(want)[ok]), w
        assert not bits_of(got)[~ok].any(), f"{w}: a null result is not zero"


def test_lookup_whole_column(gx, lib, T):
    rng = np.random.default_rng(23)
    n = 2 * T + 3
    vals = rng.standard_normal(n)
    srt = np.sort(vals)
    check_lookup(lib, srt, QS, True, [0, n], what="sorted")
    order = np.argsort(vals, kind="stable").astype(np.int32)
    check_lookup(lib, vals, QS, True, [0, n], order=order, what="order map")
    ints = rng.integers(-10**6, 10**6, n).astype(np.int32)
    check_lookup(lib, np.sort(ints), QS + [0.1, 0.9], False, [0, n], what="int32 inexact")
    f32 = np.sort(rng.standard_normal(n).astype(np.float32))
    check_lookup(lib, f32, QS + [0.1, 0.9], False, [0, n], what="float32 inexact")
    check_lookup(lib, f32, [0.5], True, [0, n], what="float32 exact")


def test_lookup_null_aware_validity(lib):
    """cudf::quantile's rule: count includes the nulls; a result is null when a row it reads is null"""
    rng = np.random.default_rng(29)
    n = 101
    vals = np.sort(rng.integers(0, 1000, n)).astype(np.int64)
    valid = rng.random(n) < 0.6
    qs = [k / 200 for k in range(0, 201, 7)]
    for begin_bit in BEGIN_BITS:
        check_lookup(lib, vals, qs, True, [0, n], valid, begin_bit, rng=rng, what=f"nulls begin {begin_bit}")
    order = rng.permutation(n).astype(np.int32)
    check_lookup(lib, vals, qs, True, [0, n], valid, 33, order=order, rng=rng, what="nulls + order")
    # linear between a valid and a null neighbour is null, lower on the valid one is not
    v2 = np.array([True, False])
    got, ok, _ = run_lookup(lib, np.array([1.0, 2.0]), [0.5], "linear", True, [0, 2], v2)
    assert not ok[0]
    got, ok, _ = run_lookup(lib, np.array([1.0, 2.0]), [0.5], "lower", True, [0, 2], v2)
    assert ok[0] and got[0] == 1.0


@pytest.mark.parametrize("nq", [1, 3])
def test_lookup_segments(lib, T, nq):
    """segments of 0, 1, 2, T and T + 1 rows, values sorted inside each with nulls behind the valid ones (the groupby layout)"""
    rng = np.random.default_rng(31)
    sizes = [0, 1, 2, T, T + 1, 0, 5, 1, 0]
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(offsets[-1])
    vals = np.zeros(n)
    valid = np.zeros(n, bool)
    counts = []
    for s, sz in enumerate(sizes):
        k = int(rng.integers(0, sz + 1)) if s != 3 else sz       # valid rows of the segment; one segment entirely valid
        if sz == 5:
            k = 0                                                 # ... and one entirely null
        counts.append(k)
        vals[offsets[s]: offsets[s] + k] = np.sort(rng.standard_normal(k))
        valid[offsets[s]: offsets[s] + k] = True
    qs = [0.5] if nq == 1 else [0.25, 0.5, 0.75]
    check_lookup(lib, vals, qs, True, offsets, valid, 1, counts=counts, rng=rng, what="segments with counts")
    check_lookup(lib, vals, qs, True, offsets, what="segments without counts")
    many = np.arange(0, 70001, 7).astype(np.int32)                # 10000 segments of 7 rows: more outputs than one workgroup
    check_lookup(lib, np.arange(70000, dtype=np.int64), qs, True, many, what="many segments")


# ------------------------------------------------------------------------------------------------ Python surface
def pandas_bound(srt, q):
    ix = qm.index(len(srt), q)
    return 8 * 2.0**-53 * max(abs(float(srt[ix[0]])), abs(float(srt[ix[1]])))


def test_column_quantile_and_median_against_pandas(gx, T):
    import pandas as pd
    _, Column, ops = gx
    rng = np.random.default_rng(37)
    n = 3 * T + 17
    for dt in ("float64", "int32", "int64", "float32"):
        vals = (rng.standard_normal(n) * 1000).astype(dt)
        valid = rng.random(n) < 0.9
        for col, live in ((Column.from_numpy(vals), vals), (Column.from_numpy(vals, valid), vals[valid])):
            s = pd.Series(live)
            srt = np.sort(live)
            qs = [0.0, 0.013, 0.25, 0.5, 0.77, 1.0]
            for interp in qm.INTERPS:
                got = col.quantile(qs, interp).to_numpy()
                for j, q in enumerate(qs):
                    if interp == "nearest" and qm.index(len(live), q)[3] == 0.5:
                        continue                                  # pandas' tie rule is not this model's
                    want = float(s.quantile(q, interpolation=interp))
                    if interp in ("linear", "midpoint"):
                        assert abs(got[j] - want) <= pandas_bound(srt, q), (dt, interp, q)
                    else:
                        assert got[j] == want, (dt, interp, q)
            assert abs(col.median() - float(s.median())) <= pandas_bound(srt, 0.5)
            assert isinstance(col.quantile(0.3), float)
    none = Column.from_numpy(np.zeros(5), np.zeros(5, bool))
    assert none.median() is None and none.quantile([0.1, 0.9]).null_count == 2
    with pytest.raises(ValueError):
        Column.from_numpy(vals).quantile(1.5)
    with pytest.raises(TypeError):
        Column.from_numpy(np.zeros(4, bool)).quantile(0.5)
    # every mode of ops.quantile agrees, exact=False keeps the dtype
    col = Column.from_numpy(rng.integers(-1000, 1000, n).astype(np.int32))
    a = ops.quantile(col, [0.2, 0.5], "linear", mode="select").to_numpy()
    b = ops.quantile(col, [0.2, 0.5], "linear", mode="sort").to_numpy()
    assert np.array_equal(a, b)
    for interp in qm.INTERPS:
        r = ops.quantile(col, [0.2, 0.5], interp, exact=False)
        assert r.dtype == np.int32
        assert np.array_equal(r.to_numpy(), ops.quantile(col, [0.2, 0.5], interp).to_numpy().astype(np.int32))


def test_quantile_sorted_and_quantiles(gx):
    _, Column, ops = gx
    rng = np.random.default_rng(41)
    vals = rng.standard_normal(1000)
    order = Column.from_numpy(np.argsort(vals, kind="stable").astype(np.int32))
    got = ops.quantile_sorted(Column.from_numpy(vals), [0.1, 0.5], "linear", order).to_numpy()
    want = qm.expected(np.sort(vals), [0.1, 0.5], "linear")[1]
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert ops.quantile_sorted(Column.from_numpy(vals[:0]), [0.5]).null_count == 1
    assert ops.quantile_sorted(Column.from_numpy(vals), []).size == 0
    with pytest.raises(ValueError):
        ops.quantile_sorted(Column.from_numpy(vals), [0.5], "linear", Column.from_numpy(np.zeros(3, np.int32)))
    a = rng.integers(0, 5, 200).astype(np.int32)
    b = rng.standard_normal(200)
    rows = ops.quantiles([Column.from_numpy(a), Column.from_numpy(b)], [0.0, 0.5, 1.0], "lower")
    o = np.lexsort((b, a))
    idx = [qm.index(200, q)[0] for q in (0.0, 0.5, 1.0)]
    assert np.array_equal(rows[0].to_numpy(), a[o][idx]) and np.array_equal(rows[1].to_numpy(), b[o][idx])
    with pytest.raises(ValueError):
        ops.quantiles([Column.from_numpy(a)], [0.5], "linear")
    with pytest.raises(ValueError):
        ops.quantiles([Column.from_numpy(a[:0])], [0.5], "nearest")


def test_dataframe_quantile_and_median_against_pandas(gx, T):
    import pandas as pd
    cudf_amd = gx[0]
    rng = np.random.default_rng(43)
    n = 2 * T + 9
    pdf = pd.DataFrame({"a": rng.standard_normal(n), "b": rng.integers(-500, 500, n).astype(np.int64), "c": rng.random(n)})
    pdf.loc[rng.random(n) < 0.2, "c"] = np.nan
    df = cudf_amd.DataFrame.from_pandas(pdf)
    for q in (0.5, [0.1, 0.9]):
        got = df.quantile(q)
        want = pdf.quantile(q)
        for name in pdf.columns:
            g = got[name].to_numpy()
            w = np.atleast_1d(want[name])
            live = np.sort(pdf[name].dropna().to_numpy())
            for j, qq in enumerate(np.atleast_1d(q)):
                assert abs(g[j] - w[j]) <= pandas_bound(live, qq), (name, qq)
    med = df.median()
    for name in pdf.columns:
        live = np.sort(pdf[name].dropna().to_numpy())
        assert abs(med[name].to_numpy()[0] - pdf[name].median()) <= pandas_bound(live, 0.5)


def groupby_frame(rng, two_keys):
    import pandas as pd
    sizes = [1, 2, 1000, 1, 997, 2, 3, 1003]
    k1 = np.repeat(np.array([7, -3, 100, 5, 42, 0, 9, 13], np.int32), sizes)
    n = len(k1)
    v = rng.standard_normal(n) * 100
    w = rng.integers(-1000, 1000, n).astype(np.float64)
    v[rng.random(n) < 0.15] = np.nan
    v[k1 == 9] = np.nan                                            # a group that is all null
    perm = rng.permutation(n)
    d = {"k": k1[perm], "v": v[perm], "w": w[perm]}
    if two_keys:
        d["k2"] = (np.arange(n) % 2).astype(np.int32)[perm]
    return pd.DataFrame(d)


@pytest.mark.parametrize("two_keys", [False, True])
def test_groupby_median_quantile_against_pandas(gx, two_keys):
    cudf_amd = gx[0]
    rng = np.random.default_rng(47)
    pdf = groupby_frame(rng, two_keys)
    by = ["k", "k2"] if two_keys else ["k"]
    df = cudf_amd.DataFrame.from_pandas(pdf)

    def compare(got, want, cols, q):
        want = want.reset_index()
        gp = got.to_pandas()
        assert len(gp) == len(want)
        for b in by:
            assert np.array_equal(gp[b].to_numpy(), want[b].to_numpy())
        for c, src in cols.items():
            g, w = gp[c].to_numpy(), want[c].to_numpy()
            assert np.array_equal(np.isnan(g), np.isnan(w)), c
            for i in np.flatnonzero(~np.isnan(w)):
                sel = np.ones(len(pdf), bool)
                for b in by:
                    sel &= pdf[b].to_numpy() == want[b].to_numpy()[i]
                live = np.sort(pdf.loc[sel, src].dropna().to_numpy())
                assert abs(g[i] - w[i]) <= pandas_bound(live, q), (c, i)

    compare(df.groupby(by).median(), pdf.groupby(by).median(), {"v": "v", "w": "w"}, 0.5)
    for q in (0.5, 0.9, 0.0):
        compare(df.groupby(by).quantile(q), pdf.groupby(by).quantile(q), {"v": "v", "w": "w"}, q)
    got = df.groupby(by).agg({"v": ["median", "sum"]})
    want = pdf.groupby(by).agg(v_median=("v", "median"), v_sum=("v", "sum"))
    compare(got, want, {"v_median": "v"}, 0.5)
    gs, ws = got.to_pandas()["v_sum"].to_numpy(), want.reset_index()["v_sum"].to_numpy()
    ok = ~np.isnan(gs)
    assert np.allclose(gs[ok], ws[ok], rtol=1e-12, atol=1e-9)


def test_cpp_quantile_binary():
    exe = os.path.join(ROOT, "tests", "cpp", "cudf_quantile_tests")
    assert os.path.exists(exe), "build the C++ tests first (make -C cudf_amd/cpp)"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "0 failed" in r.stdout
