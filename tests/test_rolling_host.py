"""CPU: cudf::rolling_window / grouped_rolling_window as far as they can be checked without a device -- exported symbols, the
argument checks of gx_rolling_window, the argument checks of the C++ surface, and a model of one tile of k_roll_tile
(cudf_amd/csrc/gx_rolling.hip: the two segmented scans over the tile's region only, the three-way rule for a cut window) checked
exhaustively against the naive loop, so the segment rule is pinned before any GPU run."""
import ctypes
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cudf_amd", "libcudf.so")
BIN = os.path.join(ROOT, "tests", "cpp", "cudf_rolling_tests")

GX_EINVAL, GX_EDTYPE = -1, -2


def _build():
    import __graft_entry__ as ge
    ge.build()


@pytest.fixture(autouse=True, scope="module")
def _the_kernel_layer_has_the_operator():
    """everything here, the model included, describes gx_rolling_window: without it there is nothing to pin"""
    _build()
    from cudf_amd import _lib
    assert hasattr(_lib.lib, "gx_rolling_window") and "gx_rolling_window" in _lib.EXPORTED


def test_libraries_export_the_rolling_api():
    syms = subprocess.check_output(["nm", "-DC", "--defined-only", LIB], text=True)
    for s in ["cudf::rolling_window(", "cudf::grouped_rolling_window("]:
        assert s in syms, f"libcudf.so does not export {s}"
    assert syms.count("cudf::rolling_window(") == 2                      # the fixed and the per-row overload
    und = subprocess.check_output(["nm", "-D", "--undefined-only", LIB], text=True)
    assert "gx_rolling_window" in und
    from cudf_amd import _lib
    for s in ("gx_rolling_window", "gx_rolling_tile_rows", "gx_rolling_max_span", "gx_rolling_set_kernel"):
        assert s in _lib.EXPORTED and hasattr(_lib.lib, s)
    assert os.path.exists(os.path.join(ROOT, "include", "cudf", "rolling.hpp"))


def test_tile_rows_and_span():
    from cudf_amd import _lib as L
    T, S = L.lib.gx_rolling_tile_rows(), L.lib.gx_rolling_max_span()
    assert T > 0 and T % 64 == 0          # a wave writes whole pairs of validity words
    assert 0 < S


def test_rolling_misuse_is_rejected_before_any_device_call():
    from cudf_amd import _lib as L
    lib = L.lib
    fake, fake2, fake3 = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000), ctypes.c_void_p(0x30000)

    def roll(dtype=L.INT64, inp=fake, valid=None, bit=0, n=10, p=2, f=1, pcol=None, fcol=None, labels=None, offsets=None, mp=1, op=L.OP_SUM,
             out=fake2, out_valid=fake3):
        return lib.gx_rolling_window(dtype, inp, valid, bit, n, p, f, pcol, fcol, labels, offsets, mp, op, out, out_valid, None, None)

    for n in (-1, 2**31, 2**40):
        assert roll(n=n) == GX_EINVAL, n
    assert roll(mp=-1) == GX_EINVAL
    assert roll(pcol=fake) == GX_EINVAL and roll(fcol=fake) == GX_EINVAL            # only one of the two window columns
    assert roll(labels=fake) == GX_EINVAL and roll(offsets=fake) == GX_EINVAL        # only one of labels / offsets
    assert roll(inp=None) == GX_EINVAL and roll(out=None) == GX_EINVAL and roll(out_valid=None) == GX_EINVAL
    assert roll(bit=-1) == GX_EINVAL
    for dt in (0, 12, 99, -3):
        assert roll(dtype=dt) == GX_EDTYPE, dt
    for op in (L.OP_PRODUCT, 6, 7, 11, -1):
        assert roll(op=op) == GX_EDTYPE, op
    # no rows: nothing is launched, whatever the pointers and the window
    for op in (L.OP_SUM, L.OP_MIN, L.OP_MAX, L.OP_MEAN, L.OP_COUNT_VALID, L.OP_COUNT_ALL):
        for dt in range(L.INT8, L.BOOL8 + 1):
            assert roll(dtype=dt, op=op, n=0, inp=None, out=None, out_valid=None, p=-2**40, f=2**40) == 0
    assert roll(n=0, pcol=fake, fcol=fake, labels=fake, offsets=fake, inp=None, out=None, out_valid=None) == 0


def test_cpp_argument_checks_run_without_a_device():
    """every throw of cudf::rolling_window / grouped_rolling_window and their empty results: decided by the C++ surface before its
    first device call (tests/cpp/cudf_rolling_tests --host)"""
    _build()
    r = subprocess.run([BIN, "--host"], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "6 run, 0 failed" in r.stdout
    assert "[ OK ] window columns that are not non-nullable INT32 of input.size() rows throw cudf::logic_error" in r.stdout


def test_python_surface_rejects_bad_arguments_without_a_device():
    import numpy as np
    from cudf_amd import Column, DataFrame, ops
    c = Column(None, np.int64, 4)
    w = Column(None, np.int32, 4)
    with pytest.raises(ValueError):
        ops.rolling_window(c, 2, 1, 1, "product")
    with pytest.raises(ValueError):
        ops.rolling_window(c, 2, 1, -1, "sum")
    with pytest.raises(ValueError):
        ops.rolling_window(c, w, 1, 1, "sum")                              # only one window column
    with pytest.raises(ValueError):
        ops.rolling_window(c, w, Column(None, np.int64, 4), 1, "sum")      # not INT32
    with pytest.raises(ValueError):
        ops.rolling_window(c, w, Column(None, np.int32, 3), 1, "sum")      # another row count
    with pytest.raises(ValueError):
        DataFrame().rolling(3, min_periods=4)
    with pytest.raises(ValueError):
        DataFrame().rolling(-1)
    r = DataFrame().rolling(4, center=True)
    assert (r._preceding, r._following, r._min_periods) == (3, 1, 4)
    r = DataFrame().rolling(5, min_periods=2, center=True)
    assert (r._preceding, r._following, r._min_periods) == (3, 2, 2)
    r = DataFrame().rolling(3)
    assert (r._preceding, r._following, r._min_periods) == (3, 0, 3)


# ------------------------------------------------------------------------------------------------ the model of one tile
# x: values, valid: flags, gs / ge: first row and end of every row's group, (p, f): the window, tile = [tile_lo, tile_lo + T).

def _naive(x, valid, gs, ge, p, f, op, rows):
    out = {}
    for i in rows:
        lo, hi = max(i - p + 1, gs[i]), min(i + f, ge[i] - 1)
        v = [x[j] for j in range(lo, hi + 1) if valid[j]]
        out[i] = (op(v) if v else None, len(v), max(hi - lo + 1, 0))
    return out


def _model_tile(x, valid, gs, ge, p, f, op2, ident, tile_lo, T):
    """k_roll_tile for the output rows [tile_lo, tile_lo + T): the scans are computed over the tile's region ONLY and start from
    nothing at its two ends.  Rows outside [0, n) are identities that start and end a group."""
    n, L = len(x), p + f
    left, right = max(p - 1, 0), max(f, 0)
    assert L >= 1
    r0, w = tile_lo - left, T + left + right
    val, cnt, head, tail = [ident] * w, [0] * w, [True] * w, [True] * w
    for k in range(w):
        row = r0 + k
        if 0 <= row < n:
            pos = (row - gs[row]) % L
            head[k] = pos == 0
            tail[k] = pos == L - 1 or row == ge[row] - 1
            if valid[row]:
                val[k], cnt[k] = x[row], 1
    pre, cp, suf, cs = [None] * w, [0] * w, [None] * w, [0] * w
    run, c = ident, 0                                   # forward: nothing before the region
    for k in range(w):
        run, c = (val[k], cnt[k]) if head[k] else (op2(run, val[k]), c + cnt[k])
        pre[k], cp[k] = run, c
    run, c = ident, 0                                   # backward: nothing behind it
    for k in range(w - 1, -1, -1):
        run, c = (val[k], cnt[k]) if tail[k] else (op2(val[k], run), c + cnt[k])
        suf[k], cs[k] = run, c
    out = {}
    for i in range(tile_lo, min(tile_lo + T, n)):
        lo, hi = max(i - p + 1, gs[i]), min(i + f, ge[i] - 1)
        size = max(hi - lo + 1, 0)
        if size == 0:
            out[i] = (None, 0, 0)
            continue
        kl, kh = lo - r0, hi - r0
        assert 0 <= kl <= kh < w                        # the region holds every cut window of the tile
        rlo = (lo - gs[i]) % L
        if rlo + size - 1 >= L:                         # lo and hi in different, necessarily adjacent, segments
            assert tail[kl + (L - 1 - rlo)] and head[kl + (L - rlo)] and kl + (L - rlo) <= kh
            v, c = op2(suf[kl], pre[kh]), cs[kl] + cp[kh]
        elif rlo == 0:
            v, c = pre[kh], cp[kh]
        else:
            assert tail[kh]
            v, c = suf[kl], cs[kl]
        out[i] = (v if c > 0 else None, c, size)
    return out


def _groups_from_cuts(n, cuts):
    gs, ge = [0] * n, [0] * n
    for a, b in zip(cuts[:-1], cuts[1:]):
        for i in range(a, b):
            gs[i], ge[i] = a, b
    return gs, ge


_OPS = ((sum, lambda a, b: a + b, 0), (min, min, 10**9), (max, max, -10**9))


def _check(x, valid, gs, ge, p, f, T):
    n = len(x)
    for op, op2, ident in _OPS:
        want = _naive(x, valid, gs, ge, p, f, op, range(n))
        got = {}
        for tile_lo in range(0, n, T):
            got.update(_model_tile(x, valid, gs, ge, p, f, op2, ident, tile_lo, T))
        assert got == want, (x, valid, gs, p, f, T, op.__name__)


def test_model_of_one_tile_against_the_naive_loop_exhaustively():
    """T = 4, 11 rows (three tiles, the last ragged), every (preceding, following) in [-3, 8]^2 with a row in the window, one group cut
    at every position and every pair of positions, three null patterns"""
    n, T = 11, 4
    x = [3, -7, 11, 2, -5, 13, -1, 17, -19, 23, 4]
    patterns = ([True] * n, [i % 3 != 1 for i in range(n)], [i in (0, 5, 6) for i in range(n)])
    cuts = [[0, n]] + [[0, a, n] for a in range(1, n)] + [[0, a, b, n] for a, b in itertools.combinations(range(1, n), 2)]
    cases = 0
    for p, f in itertools.product(range(-3, 9), repeat=2):
        if p + f < 1:
            continue
        for cut in cuts:
            gs, ge = _groups_from_cuts(n, cut)
            for valid in patterns:
                _check(x, valid, gs, ge, p, f, T)
                cases += 1
    assert cases > 15000


def test_model_other_tile_sizes_groups_of_one_and_all_null():
    import random
    rng = random.Random(5)
    for trial in range(300):
        n = rng.randint(1, 40)
        x = [rng.randint(-50, 50) for _ in range(n)]
        valid = [rng.random() < (0.0 if trial % 7 == 0 else 0.8) for _ in range(n)]
        if trial % 5 == 0:
            cut = list(range(n + 1))                     # every group one row
        else:
            cut = sorted(set([0, n] + [rng.randint(0, n) for _ in range(rng.randint(0, 5))]))
        gs, ge = _groups_from_cuts(n, cut)
        p, f = rng.randint(-5, 12), rng.randint(-5, 12)
        if p + f < 1:
            continue
        _check(x, valid, gs, ge, p, f, rng.choice((1, 2, 3, 5, 8, 16)))
