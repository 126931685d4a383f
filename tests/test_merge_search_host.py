"""CPU: cudf::merge and cudf::lower_bound / upper_bound as far as they can be checked without a device -- exported symbols, scratch
queries and argument checks of gx_merge_order / gx_gather2 / gx_search_bounds, the argument checks of the C++ surface, and a model
of the merge-path splits of cudf_amd/csrc/gx_merge.hip (the diagonal split of a tile, the split of a thread inside its tile, the
bounded serial merge, the proportional fallback) checked against the oracle, so the tie rule is pinned before any GPU run."""
import ctypes
import itertools
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import cudf_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cudf_amd", "libcudf.so")
BIN = os.path.join(ROOT, "tests", "cpp", "cudf_merge_tests")

GX_EINVAL, GX_EDTYPE, GX_ETMP = -1, -2, -3


def _build():
    import __graft_entry__ as ge
    ge.build()


def test_libraries_export_the_merge_and_search_api():
    _build()
    syms = subprocess.check_output(["nm", "-DC", "--defined-only", LIB], text=True)
    for s in ["cudf::merge(", "cudf::lower_bound(", "cudf::upper_bound("]:
        assert s in syms, f"libcudf.so does not export {s}"
    und = subprocess.check_output(["nm", "-D", "--undefined-only", LIB], text=True)
    for s in ("gx_merge_order", "gx_gather2", "gx_search_bounds"):
        assert s in und, f"libcudf.so has no reference to {s}"
    from cudf_amd import _lib
    for s in ("gx_merge_order", "gx_gather2", "gx_search_bounds", "gx_merge_tile_rows"):
        assert s in _lib.EXPORTED and hasattr(_lib.lib, s)
    for h in ("merge.hpp", "search.hpp"):
        assert os.path.exists(os.path.join(ROOT, "include", "cudf", h))


def _api():
    from cudf_amd import _lib as L
    lib = L.lib
    nb = ctypes.c_size_t(0)

    def merge(nkeys, dtypes, a_cols, na, b_cols, nb_rows, out=None, tmp=None, nbytes=0, a_bits=None, b_bits=None, desc=None, nbf=None):
        nb.value = nbytes
        rc = lib.gx_merge_order(nkeys, dtypes, a_cols, None, a_bits, na, b_cols, None, b_bits, nb_rows, desc, nbf, out, tmp, ctypes.byref(nb), None)
        return rc, nb.value

    return L, lib, merge


def test_tile_rows_and_scratch_queries_without_a_device():
    L, lib, merge = _api()
    T = lib.gx_merge_tile_rows()
    assert T >= 256 and T % 64 == 0
    i64 = (ctypes.c_int * 1)(L.INT64)
    mixed = (ctypes.c_int * 4)(L.INT8, L.FLOAT64, L.INT32, L.UINT16)
    sizes = []
    for na, nb in ((0, 0), (5, 0), (1000, 1000), (10**6, 10**6), (2**30, 2**30 - 1)):
        rc, b = merge(1, i64, None, na, None, nb)
        assert rc == 0 and b > 0, (na, nb, rc, b)
        assert b >= 4 * ((na + nb + T - 1) // T), (na, nb, b)            # one split per tile
        assert b <= 4 * ((na + nb + T - 1) // T) + 4096, (na, nb, b)      # ... and little else: the merge needs no row-sized scratch
        assert merge(4, mixed, None, na, None, nb)[1] == b                 # the key columns do not change the scratch
        assert merge(1, i64, None, nb, None, na)[1] == b                   # only the total counts
        sizes.append(b)
    assert sizes == sorted(sizes)


def test_merge_order_misuse_is_rejected_before_any_device_call():
    L, lib, merge = _api()
    i64 = (ctypes.c_int * 1)(L.INT64)
    bad = (ctypes.c_int * 2)(L.INT64, 99)
    many = (ctypes.c_int * 33)(*([L.INT32] * 33))
    neg = (ctypes.c_int64 * 1)(-1)
    zero = (ctypes.c_int64 * 1)(0)
    fake = ctypes.c_void_p(0x10000)                       # a "device pointer" that must never be dereferenced
    one_col = (ctypes.c_void_p * 1)(0x20000)
    null_col = (ctypes.c_void_p * 1)(None)
    for na, nb in ((-1, 0), (0, -1), (2**31, 0), (2**30, 2**30), (2**31 - 1, 1)):
        assert merge(1, i64, None, na, None, nb)[0] == GX_EINVAL, (na, nb)
    assert merge(1, i64, None, 2**31 - 2, None, 1)[0] == 0
    for nkeys, dts in ((0, i64), (-1, i64), (33, many)):
        assert merge(nkeys, dts, None, 10, None, 10)[0] == GX_EINVAL
    assert merge(32, many, None, 10, None, 10)[0] == 0
    assert merge(1, None, None, 10, None, 10)[0] == GX_EINVAL                      # no dtypes
    assert merge(2, bad, None, 10, None, 10)[0] == GX_EDTYPE
    assert merge(1, i64, None, 10, None, 10, a_bits=neg)[0] == GX_EINVAL           # negative begin bit
    assert merge(1, i64, None, 10, None, 10, b_bits=neg)[0] == GX_EINVAL
    assert merge(1, i64, None, 10, None, 10, a_bits=zero, b_bits=zero)[0] == 0
    assert lib.gx_merge_order(1, i64, None, None, None, 10, None, None, None, 10, None, None, None, None, None, None) == GX_EINVAL   # nowhere to put the size
    need = merge(1, i64, None, 10, None, 10)[1]
    # with scratch: null column / output pointers and short scratch are refused -- all before anything is launched
    assert merge(1, i64, None, 10, one_col, 10, fake, fake, need)[0] == GX_EINVAL
    assert merge(1, i64, one_col, 10, null_col, 10, fake, fake, need)[0] == GX_EINVAL
    assert merge(1, i64, one_col, 10, one_col, 10, None, fake, need)[0] == GX_EINVAL
    assert merge(1, i64, one_col, 10, one_col, 10, fake, fake, need - 1)[0] == GX_ETMP
    assert merge(1, i64, one_col, 10, one_col, 10, fake, fake, 0)[0] == GX_ETMP
    # nothing to merge: nothing is launched, whatever the pointers
    assert merge(1, i64, None, 0, None, 0, None, fake, merge(1, i64, None, 0, None, 0)[1])[0] == 0


def test_gather2_and_search_misuse_is_rejected_before_any_device_call():
    L, lib, _ = _api()
    fake, fake2 = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000)

    def gather2(esz, a, av, abit, na, b, bv, bbit, nb, m, n, out, ov):
        return lib.gx_gather2(esz, a, av, abit, na, b, bv, bbit, nb, m, n, out, ov, None, None)

    for esz in (0, 3, 5, 16):
        assert gather2(esz, fake, None, 0, 4, fake, None, 0, 4, fake, 8, fake, None) == GX_EDTYPE
    assert gather2(8, fake, None, 0, -1, fake, None, 0, 4, fake, 8, fake, None) == GX_EINVAL
    assert gather2(8, fake, None, 0, 4, fake, None, 0, 4, fake, -8, fake, None) == GX_EINVAL
    assert gather2(8, fake, None, 0, 2**30, fake, None, 0, 2**30, fake, 8, fake, None) == GX_EINVAL
    assert gather2(8, fake, None, -1, 4, fake, None, 0, 4, fake, 8, fake, None) == GX_EINVAL
    assert gather2(8, fake, fake2, 0, 4, fake, None, 0, 4, fake, 8, fake, None) == GX_EINVAL     # a bitmap in, none out
    assert gather2(8, fake, None, 0, 4, fake, fake2, 0, 4, fake, 8, fake, None) == GX_EINVAL
    assert gather2(8, fake, None, 0, 4, fake, None, 0, 4, None, 8, fake, None) == GX_EINVAL       # no map
    assert gather2(8, fake, None, 0, 4, fake, None, 0, 4, fake, 8, None, None) == GX_EINVAL       # no output
    assert gather2(8, None, None, 0, 4, fake, None, 0, 4, fake, 8, fake, None) == GX_EINVAL       # a side with rows and no data
    assert gather2(8, None, None, 0, 0, None, None, 0, 0, None, 0, None, None) == 0               # no rows: nothing runs

    i64 = (ctypes.c_int * 1)(L.INT64)
    bad = (ctypes.c_int * 1)(42)
    many = (ctypes.c_int * 33)(*([L.INT32] * 33))
    one_col = (ctypes.c_void_p * 1)(0x20000)
    null_col = (ctypes.c_void_p * 1)(None)
    neg = (ctypes.c_int64 * 1)(-1)

    def search(nkeys, dts, hay, nh, needles, nn, out, hbits=None, upper=0):
        return lib.gx_search_bounds(nkeys, dts, hay, None, hbits, nh, needles, None, None, nn, None, None, upper, out, None)

    assert search(1, i64, one_col, -1, one_col, 4, fake) == GX_EINVAL
    assert search(1, i64, one_col, 4, one_col, 2**31, fake) == GX_EINVAL
    assert search(0, i64, one_col, 4, one_col, 4, fake) == GX_EINVAL
    assert search(33, many, one_col, 4, one_col, 4, fake) == GX_EINVAL
    assert search(1, None, one_col, 4, one_col, 4, fake) == GX_EINVAL
    assert search(1, bad, one_col, 4, one_col, 4, fake) == GX_EDTYPE
    assert search(1, i64, one_col, 4, one_col, 4, fake, hbits=neg) == GX_EINVAL
    assert search(1, i64, None, 4, one_col, 4, fake) == GX_EINVAL
    assert search(1, i64, one_col, 4, null_col, 4, fake) == GX_EINVAL
    assert search(1, i64, one_col, 4, one_col, 4, None) == GX_EINVAL
    for upper in (0, 1):
        assert search(1, i64, one_col, 4, None, 0, None, upper=upper) == 0                        # no needles: nothing runs


def test_cpp_argument_checks_run_without_a_device():
    """every throw of cudf::merge / lower_bound / upper_bound and their empty results: decided by the C++ surface before its first
    device call (tests/cpp/cudf_merge_tests --host)"""
    _build()
    r = subprocess.run([BIN, "--host"], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "7 run, 0 failed" in r.stdout
    assert "[ OK ] merge: a key index outside the table throws std::out_of_range" in r.stdout
    assert "[ OK ] merge: a total row count beyond size_type throws std::overflow_error" in r.stdout


def test_python_surface_rejects_bad_arguments_without_a_device():
    from cudf_amd import DataFrame, ops
    assert ops.merge_sorted([], [0]) == []
    for fn in (ops.merge_order, ops.lower_bound, ops.upper_bound):
        with pytest.raises(ValueError):
            fn([], [])                     # no key columns at all
    with pytest.raises(ValueError):
        DataFrame().searchsorted([1], side="middle")
    with pytest.raises(ValueError):
        DataFrame().searchsorted([1])      # a frame without columns


# ------------------------------------------------------------------------------------------------ the merge-path model
# Rows are tuples of sortable keys (what to_sortable + the descending mask leave); the leading key sits in "LDS", the columns behind
# are looked at only when two leading keys agree -- the policy split of k_mp_merge.

def _a_first(ra, rb):
    """A's row before B's row?  A goes first unless B is STRICTLY smaller: NOT (B < A)"""
    if ra[0] != rb[0]:
        return ra[0] < rb[0]
    return not (rb[1:] < ra[1:])


def _diagonal_split(a, b, d):
    """k_mp_partition: the number of rows of a among the first d rows of the stable merge"""
    lo, hi = max(0, d - len(b)), min(d, len(a))
    while lo < hi:
        mid = (lo + hi) // 2
        assert 0 <= mid < len(a) and 0 <= d - 1 - mid < len(b)             # clamped by construction
        if _a_first(a[mid], b[d - 1 - mid]):
            lo = mid + 1
        else:
            hi = mid
    return lo


def _model_merge(a, b, tile, items):
    """gx_merge_order on rows without nulls: the map, and whether a fallback to the proportional split was taken"""
    na, nb = len(a), len(b)
    n = na + nb
    threads = tile // items
    ntiles = (n + tile - 1) // tile
    fell_back = False
    split, flag = [], False
    for t in range(ntiles):
        d0, d1 = t * tile, min(t * tile + tile, n)
        s0 = 0 if t == 0 else _diagonal_split(a, b, d0)
        s1 = na if d1 == n else _diagonal_split(a, b, d1)
        split.append(s0)
        flag |= s1 < s0 or s1 - s0 > d1 - d0
    out = [None] * n
    for t in range(ntiles):
        d0, d1 = t * tile, min(t * tile + tile, n)
        cnt = d1 - d0
        if flag:
            fell_back = True
            a0, a1 = d0 * na // n, d1 * na // n
        else:
            a0, a1 = (0 if t == 0 else split[t]), (na if d1 == n else split[t + 1])
        b0, ac = d0 - a0, a1 - a0
        bc = cnt - ac
        assert 0 <= ac <= cnt and 0 <= a0 and a0 + ac <= na and 0 <= b0 and b0 + bc <= nb
        ta, tb = a[a0:a0 + ac], b[b0:b0 + bc]                              # the tile's rows ("LDS": their leading keys)
        di = [min(i * items, cnt) for i in range(threads + 1)]
        s = []
        for i in range(threads):
            s.append(_diagonal_split(ta, tb, di[i]))
        s.append(ac)
        if any(s[i + 1] < s[i] or s[i + 1] - s[i] > di[i + 1] - di[i] for i in range(threads)):
            fell_back = True
            s = [d * ac // cnt for d in di]
        for i in range(threads):
            ia, ja, iend, jend = s[i], di[i] - s[i], s[i + 1], di[i + 1] - s[i + 1]
            for u in range(di[i + 1] - di[i]):
                if ja >= jend or (ia < iend and _a_first(ta[ia], tb[ja])):
                    out[d0 + di[i] + u] = a0 + ia
                    ia += 1
                else:
                    out[d0 + di[i] + u] = na + b0 + ja
                    ja += 1
            assert ia == iend and ja == jend
    return out, fell_back


def _sorted_vectors(n, nvalues):
    return list(itertools.combinations_with_replacement(range(nvalues), n))


def test_model_of_the_splits_against_the_oracle_exhaustively():
    """every pair of sorted key vectors with 0 .. 12 rows each and keys in [0, 3): the map of the model, whose ties sit across tile and
    thread boundaries (tile = 4 rows, 2 rows per thread), is the oracle's stable order of the concatenation a || b.  One oracle call
    orders all cases at once: a leading case number keeps them apart."""
    vecs = [v for n in range(13) for v in _sorted_vectors(n, 3)]
    cases = [(a, b) for a in vecs for b in vecs]
    case_id = np.concatenate([np.full(len(a) + len(b), c, np.int64) for c, (a, b) in enumerate(cases)])
    keys = np.concatenate([np.asarray(a + b, np.int64) for a, b in cases])
    order = orc.sorted_order_rows([case_id, keys])
    starts = np.concatenate([[0], np.cumsum([len(a) + len(b) for a, b in cases])])
    assert len(cases) == 455 * 455
    for c, (a, b) in enumerate(cases):
        got, fell_back = _model_merge([(k,) for k in a], [(k,) for k in b], 4, 2)
        want = order[starts[c]:starts[c + 1]] - starts[c]
        assert not fell_back and got == want.tolist(), (a, b, got, want.tolist())


def test_model_with_columns_behind_the_leading_key_and_other_tile_shapes():
    rng = random.Random(7)
    for trial in range(400):
        na, nb = rng.randint(0, 40), rng.randint(0, 40)
        a = sorted((rng.randrange(3), rng.randrange(2), rng.randrange(2)) for _ in range(na))
        b = sorted((rng.randrange(3), rng.randrange(2), rng.randrange(2)) for _ in range(nb))
        cols = [np.asarray([r[k] for r in a + b], np.int64) for k in range(3)]
        want = orc.sorted_order_rows(cols).tolist() if na + nb else []
        for tile, items in ((4, 2), (8, 2), (6, 3), (16, 4)):
            got, fell_back = _model_merge(a, b, tile, items)
            assert not fell_back and got == want, (a, b, tile, items)


def test_model_on_unsorted_input_still_gives_a_permutation():
    """unsorted rows: neighbouring splits can come out of order; the proportional fallback keeps every row in exactly one thread's range"""
    rng = random.Random(11)
    fallbacks = 0
    for trial in range(600):
        na, nb = rng.randint(0, 30), rng.randint(0, 30)
        a = [(rng.randrange(5),) for _ in range(na)]
        b = [(rng.randrange(5),) for _ in range(nb)]
        if trial % 3 == 0:
            a.sort()
        got, fell_back = _model_merge(a, b, 8, 2)
        fallbacks += fell_back
        assert sorted(got) == list(range(na + nb)), (a, b, got)
    assert fallbacks > 100
