"""CPU: cudf::quantile / quantiles / MEDIAN / QUANTILE as far as they can be checked without a device -- exported symbols, the scratch
query of gx_quantile, every argument check of gx_quantile and gx_quantile_lookup (fake pointers: nothing is launched), the --host
cases of the C++ surface, the shared index helper against exact rational arithmetic, and a NumPy model of the select protocol
(range, digit, histogram, plan, candidate positions: tests/quantile_model.py) checked exhaustively against np.sort."""
import ctypes
import itertools
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import quantile_model as qm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cudf_amd", "libcudf.so")
BIN = os.path.join(ROOT, "tests", "cpp", "cudf_quantile_tests")

GX_EINVAL, GX_EDTYPE, GX_ETMP = -1, -2, -3
NEW = ("gx_quantile_tile_rows", "gx_quantile_index", "gx_quantile", "gx_quantile_status", "gx_quantile_lookup",
       "gx_quantile_set_thresholds", "gx_quantile_get_thresholds")
A, B, C, D = (ctypes.c_void_p(x) for x in (0x10000, 0x20000, 0x30000, 0x40000))   # "device pointers" that are never dereferenced


def _build():
    import __graft_entry__ as ge
    ge.build()


@pytest.fixture(autouse=True, scope="module")
def _the_kernel_layer_has_the_family():
    _build()
    from cudf_amd import _lib
    assert hasattr(_lib.lib, "gx_quantile") and "gx_quantile" in _lib.EXPORTED


@pytest.fixture(scope="module")
def lib():
    from cudf_amd import _lib
    return _lib.lib


def _q(*qs):
    return (ctypes.c_double * len(qs))(*qs)


def test_libraries_export_the_quantile_api(lib):
    from cudf_amd import _lib
    for s in NEW:
        assert hasattr(lib, s) and s in _lib.EXPORTED
    syms = subprocess.check_output(["nm", "-DC", "--defined-only", LIB], text=True)
    for s in ("cudf::quantile(", "cudf::quantiles("):
        assert syms.count(s) == 1, f"libcudf.so exports {syms.count(s)} overloads of {s}"
    und = subprocess.check_output(["nm", "-D", "--undefined-only", LIB], text=True)
    for s in ("gx_quantile", "gx_quantile_lookup"):
        assert s in und
    assert lib.gx_quantile_tile_rows() > 0 and lib.gx_quantile_tile_rows() % 64 == 0


def test_scratch_query_is_host_arithmetic(lib):
    from cudf_amd import _lib as L
    nb = ctypes.c_size_t(0)

    def query(dtype, n, bitmap, mode=0):
        nb.value = 0
        rc = lib.gx_quantile(dtype, None, B if bitmap else None, 0, n, _q(0.5), 1, 0, mode, None, None, None, None, None, ctypes.byref(nb), None)
        assert rc == 0, (dtype, n, rc)
        return nb.value

    for dtype in (L.INT8, L.INT64, L.FLOAT32, L.FLOAT64):
        for bitmap in (False, True):
            sizes = [query(dtype, n, bitmap) for n in (0, 1, 1000, 10**6, 10**8, 10**9, 2**31 - 1)]
            assert sizes == sorted(sizes) and sizes[0] > 0, (dtype, bitmap, sizes)
        assert query(dtype, 10**6, True) >= query(dtype, 10**6, False)
    # two buffers of n elements beside the sort's own scratch
    assert query(L.INT64, 10**9, False) > 16 * 10**9


def test_gx_quantile_argument_checks(lib):
    from cudf_amd import _lib as L
    nb = ctypes.c_size_t(1 << 40)
    path = ctypes.c_int(0)

    def call(dtype=L.INT64, data=A, valid=None, bit0=0, n=100, q=_q(0.5), nq=1, interp=0, mode=0, f64=B, elems=None, nvalid=C, tmp=D,
             tb=ctypes.byref(nb)):
        return lib.gx_quantile(dtype, data, valid, bit0, n, q, nq, interp, mode, f64, elems, nvalid, ctypes.byref(path), tmp, tb, None)

    assert call(dtype=L.BOOL8) == GX_EDTYPE
    assert call(dtype=99) == GX_EDTYPE
    assert call(dtype=0) == GX_EDTYPE
    assert call(n=-1) == GX_EINVAL
    assert call(n=2**31) == GX_EINVAL
    assert call(nq=0) == GX_EINVAL
    assert call(nq=65, q=_q(*([0.5] * 65))) == GX_EINVAL
    assert call(q=None) == GX_EINVAL
    assert call(q=_q(float("nan"))) == GX_EINVAL
    assert call(interp=-1) == GX_EINVAL and call(interp=5) == GX_EINVAL
    assert call(mode=-1) == GX_EINVAL and call(mode=3) == GX_EINVAL
    assert call(bit0=-1, valid=B) == GX_EINVAL
    assert call(tb=None) == GX_EINVAL
    assert call(f64=None) == GX_EINVAL
    assert call(nvalid=None) == GX_EINVAL
    assert call(data=None) == GX_EINVAL
    small = ctypes.c_size_t(64)
    assert call(tb=ctypes.byref(small)) == GX_ETMP
    # q outside [0, 1] is clamped, not refused: the query still answers
    nb2 = ctypes.c_size_t(0)
    assert call(q=_q(-3.0, 7.0), nq=2, tmp=None, tb=ctypes.byref(nb2)) == 0 and nb2.value > 0


def test_gx_quantile_lookup_argument_checks(lib):
    from cudf_amd import _lib as L

    def call(dtype=L.FLOAT64, data=A, valid=None, bit0=0, order=None, nseg=1, offsets=B, counts=None, q=_q(0.5), nq=1, interp=0, exact=1,
             out=C, out_valid=None, nulls=None):
        return lib.gx_quantile_lookup(dtype, data, valid, bit0, order, nseg, offsets, counts, q, nq, interp, exact, out, out_valid, nulls, None)

    assert call(dtype=L.BOOL8) == GX_EDTYPE
    assert call(dtype=42) == GX_EDTYPE
    assert call(nseg=-1) == GX_EINVAL
    assert call(nseg=2**31 // 2, nq=2, q=_q(0.1, 0.2)) == GX_EINVAL
    assert call(nq=0) == GX_EINVAL and call(nq=65, q=_q(*([0.5] * 65))) == GX_EINVAL
    assert call(q=None) == GX_EINVAL
    assert call(q=_q(float("nan"))) == GX_EINVAL
    assert call(interp=5) == GX_EINVAL
    assert call(bit0=-1) == GX_EINVAL
    assert call(offsets=None) == GX_EINVAL
    assert call(out=None) == GX_EINVAL


def test_thresholds_round_trip(lib):
    mr, sh = ctypes.c_int64(0), ctypes.c_double(0)
    lib.gx_quantile_get_thresholds(ctypes.byref(mr), ctypes.byref(sh))
    d_mr, d_sh = mr.value, sh.value
    assert d_mr > 0 and 0.0 < d_sh <= 1.0
    try:
        lib.gx_quantile_set_thresholds(12345, 0.5)
        lib.gx_quantile_get_thresholds(ctypes.byref(mr), ctypes.byref(sh))
        assert (mr.value, sh.value) == (12345, 0.5)
    finally:
        lib.gx_quantile_set_thresholds(-1, -1.0)
    lib.gx_quantile_get_thresholds(ctypes.byref(mr), ctypes.byref(sh))
    assert (mr.value, sh.value) == (d_mr, d_sh)


def test_header_declares_the_family_as_c99():
    src = '#include "cudf_amd/gx_knobs.h"\nint main(void) { return GX_QUANTILE_PATH_SORT == 3 && GX_INTERP_NEAREST == 4 ? 0 : 1; }\n'
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_cpp_host_cases_run_without_a_device():
    """the throws of the C++ surface and the empty results: decided before the first device call"""
    _build()
    r = subprocess.run([BIN, "--host"], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert ", 0 failed" in r.stdout
    assert "[ OK ] quantiles with an arithmetic interpolation throws" in r.stdout


# ---------------------------------------------------------------------------------------------------------------------
# the index helper, against exact rationals
# ---------------------------------------------------------------------------------------------------------------------
Q_GRID = sorted(set([0.0, 1.0, 0.5, 0.25, 0.75, 1e-9, 1 - 1e-9, 1 / 3, 2 / 3, 0.1, 0.9, 0.01, 0.99, 5e-324, np.nextafter(1.0, 0.0),
                     np.nextafter(0.5, 0.0), np.nextafter(0.5, 1.0)] + [k / 64 for k in range(65)] + [k / 7 for k in range(8)]))


def _exact_index(count, q):
    pos = Fraction(float(Fraction(q) * (count - 1)))      # the one rounding of q * (count - 1)
    lower = pos.numerator // pos.denominator
    higher = -((-pos.numerator) // pos.denominator)
    return lower, higher, round(pos), float(pos - lower)  # round(Fraction) is half-to-even; the difference is exact


def test_index_helper_against_fractions(lib):
    lo, hi, ne = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
    fr = ctypes.c_double(0.0)
    ties = 0
    for count in range(1, 65):
        for q in Q_GRID:
            assert lib.gx_quantile_index(count, q, ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(ne), ctypes.byref(fr)) == 0
            want = _exact_index(count, q)
            assert (lo.value, hi.value, ne.value, fr.value) == want, (count, q)
            assert 0 <= lo.value <= hi.value <= count - 1 and ne.value in (lo.value, hi.value)
            assert qm.index(count, q) == want, (count, q)
            ties += want[3] == 0.5
    assert ties > 50                                       # the half-to-even rule was exercised
    # clamped outside [0, 1]; refused for count < 1 and NaN
    assert lib.gx_quantile_index(10, -1.0, ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(ne), ctypes.byref(fr)) == 0 and hi.value == 0
    assert lib.gx_quantile_index(10, 2.0, ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(ne), ctypes.byref(fr)) == 0 and lo.value == 9
    assert lib.gx_quantile_index(0, 0.5, ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(ne), ctypes.byref(fr)) == GX_EINVAL
    assert lib.gx_quantile_index(3, float("nan"), ctypes.byref(lo), ctypes.byref(hi), ctypes.byref(ne), ctypes.byref(fr)) == GX_EINVAL


# ---------------------------------------------------------------------------------------------------------------------
# the select protocol, against np.sort
# ---------------------------------------------------------------------------------------------------------------------
def _check_plan(words):
    words = np.asarray(words, dtype=np.uint64)
    srt = np.sort(words)
    n = len(words)
    ranks = list(range(n)) if n <= 40 else sorted(set([0, 1, n // 4, n // 2, n // 2 + 1, n - 2, n - 1]))
    plan = qm.select_plan(words, ranks)
    assert plan["word"] == [int(srt[r]) for r in ranks]
    span = int(srt[-1]) - int(srt[0])
    assert plan["direct"] == (span < qm.NBINS)
    if not plan["direct"]:
        assert plan["shift"] == span.bit_length() - 11 and (span >> plan["shift"]) in range(1024, 2048)
        assert plan["c"] == len(plan["cand"]) and all(p < plan["c"] for p in plan["pos"])
    # a single rank needs one bin only: the candidates are at most the fullest bin
    one = qm.select_plan(words, [n // 2])
    assert one["word"] == [int(srt[n // 2])]
    return plan


def test_select_model_exhaustive_small():
    for n in range(1, 7):
        for tup in itertools.product(range(4), repeat=n):          # spans 0 .. 3: the plan alone answers
            assert _check_plan(tup)["direct"]
    rng = np.random.default_rng(1)
    top = (1 << 64) - 1
    for span in (0, 1, 2047, 2048, 2049, 4095, 4096, 1 << 20, (1 << 63) - 1, 1 << 63, top):
        for base in (0, 1, 12345, top - span):
            if base < 0 or base + span > top:
                continue
            for n in (1, 2, 3, 7, 40, 500):
                for trial in range(3):
                    off = [int(x) for x in rng.integers(0, span, n, dtype=np.uint64, endpoint=True)] if span else [0] * n
                    if n >= 2:
                        off[0], off[-1] = 0, span                       # both ends present: the span is the planned one
                    if trial == 1 and n >= 3:
                        off[1:-1] = [off[1]] * (n - 2)                  # one heavy value between the ends
                    if trial == 2 and n >= 3:
                        off[1:-1] = [span - min(span, k) for k in range(n - 2)]  # a cluster at the top end
                    _check_plan(np.array([base + o for o in off], dtype=np.uint64))


def test_select_model_outlier_puts_every_row_in_one_bin():
    """one outlier at each extreme stretches the span: the other rows share a bin, the candidate count is (nearly) n -- what makes
    AUTO take the sort path"""
    rng = np.random.default_rng(2)
    vals = rng.integers(100, 10001, 5000).astype(np.int64)
    vals[17], vals[4000] = np.iinfo(np.int64).min, np.iinfo(np.int64).max
    words = qm.sortable_words(vals)
    plan = qm.select_plan(words, [2499, 2500])
    assert not plan["direct"] and plan["c"] >= 4998
    assert plan["word"] == [int(x) for x in np.sort(words)[[2499, 2500]]]


def test_sortable_words_order_is_the_sort_order():
    f = np.array([0.0, -0.0, 1.5, -1.5, np.inf, -np.inf, np.nan, -np.nan, 1e-40, -1e-40, 1e30], dtype=np.float64)
    for dt in (np.float64, np.float32):
        a = f.astype(dt)
        w = qm.sortable_words(a)
        assert w[0] == w[1] and w[6] == w[7] == (1 << (8 * a.itemsize)) - 1
        order = np.argsort(w, kind="stable")
        got = a[order]
        assert np.all(np.isnan(got[-2:])) and got[0] == -np.inf and got[-3] == np.inf
        finite = got[:-2]
        assert np.all(finite[:-1] <= finite[1:])
    for dt in (np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64):
        info = np.iinfo(dt)
        a = np.array([info.min, info.max, 0, 1, info.max - 1, info.min + 1], dtype=dt)
        assert np.array_equal(a[np.argsort(qm.sortable_words(a), kind="stable")], np.sort(a))
