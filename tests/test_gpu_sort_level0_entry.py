"""GPU: the plan words that level 0 of the cursor-path sort reads ONCE, at the kernel's entry (gx_sort.hip: Level0Words, k_level0,
k_hf_scatter<.., 0, 8>).  The form that runs, the level-0 digit (HybridPlan::shift0) and the sign fold (HybridPlan::fold) are read
with scalar loads before the first key load and handed to the tile code as values.  What can go wrong is a stale or wrong word:
a digit taken at another position, a fold that is applied but no longer verified on every key, a form picked from the wrong word.

Every case: bit for bit against the plain-C oracle (int64) or cudf_oracle.sort_keys (uint64, float64), with the path pinned through
gx_sort_cursor_state / gx_sort_split_info, and the sign fold read where the device keeps it: HybridPlan::fold, at byte HY_FOLD_BYTE
of the sort's scratch (the plan is the scratch's first bytes; a static_assert next to SortPlan in gx_sort.hip holds the same number).

  sign fold and hidden keys   int64 in [-2^44, 2^44): fold on, ascending and descending; the same column with ONE key 2^60 at a row the
                              sample cannot see, at an even and at an odd row: the exact fold check must see it, level 0 declines
                              (state 2), the result is exact; keys confined to 40 bits plus one unsampled key with bit 50 set: exact
                              whatever path the device then takes
  plain keys, fold off        full-range int64 descending, full-range uint64
  float64                     N(0, 1) without NaN: splitter form, state 3; one unsampled NaN at an even and at an odd row: state 2, exact

Level 0 reads the caller's column with plain 8-byte loads (the 16-byte non-temporal pair was measured and not taken), so there is no
alignment variant here; tests/test_gpu_sort_level0_one_launch.py sorts from 8-byte-aligned columns.

Sizes: the cursor path starts at 2^25 rows.  2^25 + 1: a one-row last tile of the bit-digit form; 40 000 003: part-filled last tiles.
One input and one oracle sort per (kind, size); a column with one key replaced expects the base result with that one key replaced
(checked against the oracle itself on a small column below).  The hidden keys sit at the last unsampled rows of either parity: in the
last tile, or in the one before it where the last tile is a single row.

Wall time of the file on an MI355X: 30 s for its 23 tests, most of it the four stable-argsort oracle sorts of uint64 and float64
(4 - 6 s each, inside the first case that asks for the input); every other case takes under a second.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import c_oracle
from oracle import cudf_oracle as orc

HF_TILE = 512 * 16    # keys per tile of the bit-digit form
SAMPLE_STEP = 8 * 64  # below 2^27 rows the sample reads the 64-key chunk at every multiple of 512 rows
HY_FOLD_BYTE = 98656  # offsetof(SortPlan, hy) + offsetof(HybridPlan, fold): gx_sort.hip asserts the same constant
SIZES = {"bit_one_row_tail": 4096 * HF_TILE + 1, "odd": 40_000_003}


@pytest.fixture(scope="module")
def gx():
    import torch
    assert torch.cuda.is_available()
    import cudf_amd  # noqa: F401
    from cudf_amd import Column, ops, _lib as L
    yield Column, ops, L


def _sort(gx, v, descending=False):
    """gx_sort_keys through the C ABI -> (sorted numpy array, cursor-path state, splitter mode on, HybridPlan::fold)"""
    import torch
    Column, ops, L = gx
    col = Column.from_numpy(v)
    out = Column.empty(v.dtype, v.size)
    tmp = ops._run(L.lib.gx_sort_keys, col.gx, ctypes.c_void_p(col.data.data_ptr()), ctypes.c_void_p(out.data.data_ptr()), v.size, int(descending))
    ops._check_sort_status(tmp)
    st = ctypes.c_int32(-1)
    L.check(L.lib.gx_sort_cursor_state(ops.ptr(tmp), ctypes.byref(st), ops.stream_ptr()), "gx_sort_cursor_state")
    split = (ctypes.c_int32 * 4)()
    L.check(L.lib.gx_sort_split_info(ops.ptr(tmp), split, ops.stream_ptr()), "gx_sort_split_info")
    fold = int(tmp[HY_FOLD_BYTE:HY_FOLD_BYTE + 4].view(torch.int32).item())
    return out.to_numpy(), st.value, int(split[0]), fold


def _make(kind, n):
    rng = np.random.default_rng([n, sum(kind.encode())])
    if kind == "fold44":      # signed keys spread around zero: bits 44 .. 62 are copies of the sign
        return rng.integers(-2**44, 2**44, n, dtype=np.int64)
    if kind == "bits40":
        return rng.integers(0, 2**40, n, dtype=np.int64)
    if kind == "i64_full":
        return rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
    if kind == "u64_full":
        return rng.integers(0, 2**64 - 1, n, dtype=np.uint64)
    if kind == "f64_normal":  # N(0, 1) doubles: both signs, no NaN, no zero of either sign
        v = rng.standard_normal(n)
        v[v == 0] = 1.0
        return v
    raise AssertionError(kind)


def _oracle(v):
    return c_oracle.sort_i64(v) if v.dtype == np.int64 else orc.sort_keys(v)


def _replaced(asc, old, new):
    """the ascending result of a column in which ONE copy of `old` became `new` (new: a number above none / all of its ties' payloads
    -- distinct from every other key here -- or NaN, which cudf::sort puts last)"""
    rest = np.delete(asc, int(np.searchsorted(asc, old)))
    at = rest.size if new != new else int(np.searchsorted(rest, new))
    return np.insert(rest, at, new)


def _hidden_row(n, odd):
    """the last row of the wanted parity that no sampled chunk holds"""
    row = n - 1
    while row % SAMPLE_STEP < 64 or row % 2 != int(odd):
        row -= 1
    assert n - row <= HF_TILE + 1
    return row


class _Inputs:
    """the (column, ascending oracle result) of ONE kind at a time, both sizes: the tests below go kind by kind, so every input is
    generated and sorted by the oracle once and at most two are alive.  Descending expectations of integer keys are the reversed
    ascending result: equal integer keys are bit-identical."""

    def __init__(self):
        self.kind = None
        self.have = {}

    def get(self, kind, size):
        if self.kind != kind:
            self.kind, self.have = kind, {}
        if size not in self.have:
            v = _make(kind, SIZES[size])
            asc = _oracle(v)
            for a in (v, asc):
                a.setflags(write=False)
            self.have[size] = (v, asc)
        return self.have[size]


@pytest.fixture(scope="module")
def inputs():
    return _Inputs()


def test_expectation_shortcuts_are_the_oracles_own():
    v = np.random.default_rng(1).integers(-50, 50, 100_000, dtype=np.int64)
    asc = c_oracle.sort_i64(v)
    assert c_oracle.sort_i64(v, descending=True).tobytes() == asc[::-1].tobytes()
    w = v.copy()
    w[777] = 1 << 60
    assert c_oracle.sort_i64(w).tobytes() == _replaced(asc, v[777], np.int64(1 << 60)).tobytes()
    f = np.random.default_rng(2).standard_normal(100_000)
    fasc = orc.sort_keys(f)
    g = f.copy()
    g[4242] = np.nan
    assert orc.sort_keys(g).tobytes() == _replaced(fasc, f[4242], np.nan).tobytes()
    for n in SIZES.values():
        for odd in (False, True):
            r = _hidden_row(n, odd)
            assert r % 2 == int(odd) and r % SAMPLE_STEP >= 64


# ---- the sign fold: on, verified on every key, and declined when one hidden key breaks it
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("size", list(SIZES))
def test_sign_fold_on(gx, inputs, size, descending):
    v, asc = inputs.get("fold44", size)
    got, state, split, fold = _sort(gx, v, descending)
    print(f"{size} n={v.size} fold44 descending={descending}: state {state} split {split} fold {fold}")
    assert got.tobytes() == (asc[::-1] if descending else asc).tobytes()
    assert state == 3 and split == 0, (state, split)   # the bit-digit form of level 0 sorted the column
    assert fold == 1, fold                             # ... with (sign << 7) | seven bits as its digit


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("size", list(SIZES))
def test_sign_fold_broken_by_a_hidden_key(gx, inputs, size, odd):
    base, asc = inputs.get("fold44", size)
    row = _hidden_row(base.size, odd)
    v = base.copy()
    v[row] = 1 << 60
    got, state, split, fold = _sort(gx, v)
    print(f"{size} n={v.size} fold44 + 2^60 at row {row}: state {state} split {split} fold {fold}")
    assert got.tobytes() == _replaced(asc, base[row], np.int64(1 << 60)).tobytes()
    assert state == 2, state   # accepted by the sample, declined by level 0: the exact fold_x check saw the key


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("size", list(SIZES))
def test_exact_masks_see_a_hidden_key(gx, inputs, size, odd):
    base, asc = inputs.get("bits40", size)
    row = _hidden_row(base.size, odd)
    v = base.copy()
    v[row] = base[row] | (1 << 50)
    got, state, split, fold = _sort(gx, v)
    print(f"{size} n={v.size} bits40 + bit 50 at row {row}: state {state} split {split} fold {fold}")
    assert got.tobytes() == _replaced(asc, base[row], v[row]).tobytes()   # whatever path the device took


# ---- plain key types, fold off
@pytest.mark.parametrize("size", list(SIZES))
def test_full_range_int64_descending(gx, inputs, size):
    v, asc = inputs.get("i64_full", size)
    got, state, split, fold = _sort(gx, v, True)
    print(f"{size} n={v.size} i64_full descending: state {state} split {split} fold {fold}")
    assert got.tobytes() == asc[::-1].tobytes()
    assert state == 3 and split == 0 and fold == 0, (state, split, fold)


@pytest.mark.parametrize("size", list(SIZES))
def test_full_range_uint64(gx, inputs, size):
    v, asc = inputs.get("u64_full", size)
    got, state, split, fold = _sort(gx, v)
    print(f"{size} n={v.size} u64_full: state {state} split {split} fold {fold}")
    assert got.tobytes() == asc.tobytes()
    assert state == 3 and split == 0 and fold == 0, (state, split, fold)


# ---- float64: the splitter form, and one NaN the sample cannot see
@pytest.mark.parametrize("size", list(SIZES))
def test_doubles_without_nan(gx, inputs, size):
    v, asc = inputs.get("f64_normal", size)
    got, state, split, _ = _sort(gx, v)
    print(f"{size} n={v.size} f64_normal: state {state} split {split}")
    assert got.tobytes() == asc.tobytes()
    assert state == 3 and split == 1, (state, split)


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("size", list(SIZES))
def test_doubles_with_an_unsampled_nan(gx, inputs, size, odd):
    base, asc = inputs.get("f64_normal", size)
    row = _hidden_row(base.size, odd)
    v = base.copy()
    v[row] = np.nan
    got, state, split, _ = _sort(gx, v)
    print(f"{size} n={v.size} f64_normal + NaN at row {row}: state {state} split {split}")
    assert got.tobytes() == _replaced(asc, base[row], np.nan).tobytes()
    assert state == 2, state   # accepted by the sample, declined by level 0
