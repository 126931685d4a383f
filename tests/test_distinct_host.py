"""CPU: the deduplication feature (unique / distinct / stable_distinct / distinct_indices / the counts) as far as it can be checked
without a device -- exported symbols, scratch queries and argument checks of gx_select_unique / gx_select_distinct, the argument
checks of the C++ surface, and a model of the slot protocol of cudf_amd/csrc/gx_distinct.hip under random interleavings."""
import ctypes
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cudf_amd", "libcudf.so")
BIN = os.path.join(ROOT, "tests", "cpp", "cudf_distinct_tests")

GX_EINVAL, GX_EDTYPE, GX_ETMP = -1, -2, -3
ANY, FIRST, LAST, NONE = range(4)
SELECTORS = ("gx_select_unique", "gx_select_distinct")


def _build():
    import __graft_entry__ as ge
    ge.build()


def test_host_library_exports_the_deduplication_api():
    _build()
    syms = subprocess.check_output(["nm", "-DC", "--defined-only", LIB], text=True)
    for s in ["cudf::distinct(", "cudf::stable_distinct(", "cudf::unique(", "cudf::distinct_indices(", "cudf::distinct_count(",
              "cudf::unique_count("]:
        assert s in syms, f"libcudf.so does not export {s}"
    und = subprocess.check_output(["nm", "-D", "--undefined-only", LIB], text=True)
    for s in SELECTORS:
        assert s in und, f"libcudf.so has no reference to {s}"
    from cudf_amd import _lib
    for s in SELECTORS + ("gx_distinct_set_hash_bits",):
        assert s in _lib.EXPORTED and hasattr(_lib.lib, s)


def _api():
    from cudf_amd import _lib as L
    lib = L.lib
    nb = ctypes.c_size_t(0)

    def call(name, nkeys, dtypes, cols, valids, begins, n, keep, flags, tmp=None, nbytes=0):
        nb.value = nbytes
        rc = getattr(lib, name)(nkeys, dtypes, cols, valids, begins, n, keep, flags, None, tmp, ctypes.byref(nb), None)
        return rc, nb.value

    return L, lib, call


def _capacity(n):
    c = 64
    while c < 2 * n:
        c *= 2
    return c


def test_scratch_queries_without_a_device():
    L, lib, call = _api()
    i64 = (ctypes.c_int * 1)(L.INT64)
    mixed = (ctypes.c_int * 4)(L.INT8, L.FLOAT64, L.INT32, L.UINT16)
    rows = (0, 1000, 10**6, 2**31 - 1)
    for name in SELECTORS:
        for keep in (ANY, FIRST, LAST, NONE):
            sizes = []
            for n in rows:
                rc, b = call(name, 1, i64, None, None, None, n, keep, 3)
                assert rc == 0, (name, keep, n, rc)
                plan = lib.gx_compact_plan_bytes(n)
                assert b >= plan > 0, (name, keep, n, b, plan)
                if name == "gx_select_distinct":
                    assert b >= plan + 4 * _capacity(n), (keep, n, b)      # the plan in front, the table of row indices behind it
                else:
                    assert b == plan, (keep, n, b)                         # a streaming predicate: the plan and nothing else
                assert call(name, 4, mixed, None, None, None, n, keep, 0)[1] == b   # the key columns do not change the scratch
                sizes.append(b)
            assert sizes == sorted(sizes), (name, keep, sizes)
    # capacity: the power of two >= 2 n -- exactly 2 n at 65 536 rows, doubled one row later
    at = {n: call("gx_select_distinct", 1, i64, None, None, None, n, ANY, 3)[1] - lib.gx_compact_plan_bytes(n) for n in (65536, 65537)}
    assert at[65536] == 4 * 131072 and at[65537] == 4 * 262144


def test_misuse_is_rejected_before_any_device_call():
    L, lib, call = _api()
    i64 = (ctypes.c_int * 1)(L.INT64)
    bad = (ctypes.c_int * 2)(L.INT64, 99)
    many = (ctypes.c_int * 33)(*([L.INT32] * 33))
    neg = (ctypes.c_int64 * 1)(-1)
    zero = (ctypes.c_int64 * 1)(0)
    fake = ctypes.c_void_p(0x10000)                       # a "device pointer" that must never be dereferenced
    one_col = (ctypes.c_void_p * 1)(0x20000)
    null_col = (ctypes.c_void_p * 1)(None)
    for name in SELECTORS:
        for n in (-1, 2**31):
            assert call(name, 1, i64, None, None, None, n, ANY, 3)[0] == GX_EINVAL
        assert call(name, 1, i64, None, None, None, 2**31 - 1, ANY, 3)[0] == 0
        for nkeys, dts in ((0, i64), (-1, i64), (33, many)):
            assert call(name, nkeys, dts, None, None, None, 10, ANY, 3)[0] == GX_EINVAL
        assert call(name, 32, many, None, None, None, 10, ANY, 3)[0] == 0
        for keep in (-1, 4, 100):
            assert call(name, 1, i64, None, None, None, 10, keep, 3)[0] == GX_EINVAL
        for flags in (-1, 16, 255):
            assert call(name, 1, i64, None, None, None, 10, FIRST, flags)[0] == GX_EINVAL
        for flags in range(16):
            assert call(name, 1, i64, None, None, None, 10, FIRST, flags)[0] == 0
        assert call(name, 1, i64, None, None, neg, 10, ANY, 3)[0] == GX_EINVAL            # negative begin bit
        assert call(name, 1, i64, None, None, zero, 10, ANY, 3)[0] == 0
        assert call(name, 1, None, None, None, None, 10, ANY, 3)[0] == GX_EINVAL           # no dtypes
        assert call(name, 2, bad, None, None, None, 10, ANY, 3)[0] == GX_EDTYPE
        assert getattr(lib, name)(1, i64, None, None, None, 10, ANY, 3, None, None, None, None) == GX_EINVAL   # nowhere to put the size
        need = call(name, 1, i64, None, None, None, 10, NONE, 3)[1]
        # with scratch: null column pointers are refused, short scratch is refused -- both before anything is launched
        assert call(name, 1, i64, None, None, None, 10, NONE, 3, fake, need)[0] == GX_EINVAL
        assert call(name, 1, i64, null_col, None, None, 10, NONE, 3, fake, need)[0] == GX_EINVAL
        assert call(name, 1, i64, one_col, None, None, 10, NONE, 3, fake, need - 1)[0] == GX_ETMP
        assert call(name, 1, i64, one_col, None, None, 10, NONE, 3, fake, 0)[0] == GX_ETMP


def test_cpp_argument_checks_run_without_a_device():
    """key index out of range, more than 32 keys, no rows -> copies and zero counts: decided by the C++ surface before its first
    device call (tests/cpp/cudf_distinct_tests --host)"""
    _build()
    r = subprocess.run([BIN, "--host"], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "0 failed" in r.stdout and "[ OK ] more than 32 key columns throw std::invalid_argument" in r.stdout
    assert "[ OK ] a key index out of range" in r.stdout and "[ OK ] no rows: a copy of the input" in r.stdout


def test_python_surface_rejects_bad_arguments_without_a_device():
    from cudf_amd import ops
    with pytest.raises(ValueError):
        ops.distinct([], [], keep="middle")
    with pytest.raises(ValueError):
        ops.unique([], [], keep="NONE")
    with pytest.raises(ValueError):
        ops.distinct_indices([], keep="each")
    with pytest.raises(IndexError):
        ops.distinct([], [0])
    assert ops.stable_distinct is ops.distinct
    assert ops.distinct([], []) == [] and ops.distinct_count([]) == 0 and ops.unique_count([]) == 0


# ------------------------------------------------------------------------------------------------ the slot protocol
class _Table:
    """rep[] / hi[] of gx_distinct.hip with its atomics as single steps; rows are generators that yield between their atomics, a
    scheduler interleaves them at random"""

    def __init__(self, capacity):
        self.rep = [-1] * capacity
        self.hi = [-1] * capacity
        self.mask = capacity - 1

    def insert(self, i, key_of, home, keep, out):
        s = home & self.mask
        while True:
            r = self.rep[s]                               # the look before the CAS (may be stale by the time it is used)
            yield
            if r == -1:
                r = self.rep[s]                           # atomicCAS(&rep[s], -1, i)
                if r == -1:
                    self.rep[s] = i
                yield
            if r == -1:
                if keep == NONE:
                    self.hi[s] = max(self.hi[s], i)       # atomicMax
                    yield
                out[i] = (s, True)
                return
            if key_of[r] == key_of[i]:                    # through the key columns: the slot's class, whichever member r is
                if keep != ANY:
                    if keep in (FIRST, NONE) and i < r:
                        self.rep[s] = min(self.rep[s], i)     # atomicMin
                        yield
                    if keep == LAST and i > r:
                        self.rep[s] = max(self.rep[s], i)     # atomicMax
                        yield
                    if keep == NONE:
                        self.hi[s] = max(self.hi[s], i)
                        yield
                out[i] = (s, False)
                return
            s = (s + 1) & self.mask


@pytest.mark.parametrize("keep", [ANY, FIRST, LAST, NONE])
def test_slot_protocol_under_random_interleavings(keep):
    """several rows of one class (and of colliding classes) insert concurrently: whatever the interleaving, a class ends on ONE slot,
    rep[slot] is its smallest row (FIRST / NONE) or its largest (LAST), rep == hi iff the class has one member, and under KEEP_ANY
    exactly one row of the class claimed the slot"""
    rng = random.Random(1234 + keep)
    for trial in range(300):
        nrows = rng.randint(1, 12)
        nclasses = rng.randint(1, 4)
        key_of = [rng.randrange(nclasses) for _ in range(nrows)]
        if trial % 3 == 0:
            key_of = [0] * nrows                          # every row of one class: all contend on one slot
        same_home = trial % 2 == 0                        # every class starts at slot 0: probing runs through other classes' slots
        t = _Table(32)                                    # >= 2 nrows slots
        out = {}
        live = [t.insert(i, key_of, 0 if same_home else 7 * key_of[i] + 3, keep, out) for i in range(nrows)]
        while live:
            g = rng.choice(live)
            try:
                next(g)
            except StopIteration:
                live.remove(g)
        members = {}
        for i, k in enumerate(key_of):
            members.setdefault(k, []).append(i)
        assert sum(1 for r in t.rep if r != -1) == len(members)
        for k, rows in members.items():
            slots = {out[i][0] for i in rows}
            assert len(slots) == 1, (trial, key_of)
            s = slots.pop()
            assert sum(1 for i in rows if out[i][1]) == 1           # one claimed it, the others found it taken
            if keep == ANY:
                assert t.rep[s] in rows
            elif keep == LAST:
                assert t.rep[s] == max(rows)
            else:
                assert t.rep[s] == min(rows)
            if keep == NONE:
                assert t.hi[s] == max(rows)
                assert (t.rep[s] == t.hi[s]) == (len(rows) == 1)
            # what the second pass selects: rep[slot_of[i]] == i (and hi[...] == i)
            kept = [i for i in rows if t.rep[s] == i and (keep != NONE or t.hi[s] == i)]
            want = {ANY: None, FIRST: [min(rows)], LAST: [max(rows)], NONE: rows if len(rows) == 1 else []}[keep]
            if want is not None:
                assert kept == want
