"""GPU: what the cell kernel and level 1 of the cursor-path sort ask memory for BEFORE their key loads, and the key loads themselves
(gx_sort.hip: CellWords / cell_words, cell_meta and local_place_cell; Level1Words and the region lookup of hf_scatter_tile).
k_local_place reads its plan words once at the kernel's entry and hands them to every cell as values, and asks for a cell's size,
output position and slot in one batch.  Level 1 reads its plan words at the entry too, loads a thread's four region-table entries and
the one behind them together, then the region's start and size and the bucket's slot words in one further batch.  (16-byte key loads
of the cell kernel were built with these tests and measured; they lost and are not in the source.  The cases that aim at them -- part
filled cells, odd cell sizes, 8-byte-aligned buffers -- stay: they hold for any load width.)

What can go wrong: a plan word that is stale for a later cell of a walking workgroup, a slot computed from the wrong bucket's words,
a region found by the wrong thread or an empty region that matches, a wide load of the region table past its end or on a wrong boundary.

Every case: bit for bit against the plain-C oracle (int64) or cudf_oracle.sort_keys (every other type), one oracle sort per input, the
path pinned through gx_sort_cursor_state / gx_sort_split_info / gx_sort_place_info where the input decides it.  Knobs are restored in a
`finally`.  The cursor path starts at 2^25 rows; the look-back cases run below it on purpose.

  full-range int64            2^25 + 1 (a one-row last tile) and 40 000 003 rows (part-filled cells and tiles: odd and even cell sizes),
                              ascending and descending: state 3, splitters off
  several cells a workgroup   the 2^25 + 1 column with gx_sort_set_place_grid(1000): 1000 workgroups walk the 2^17 cells
  look-back only              2^22 + 3 and 2^23 + 12 345 rows with the cursor path off: fixed slots (ccap == 0), a bounded grid, no level 1 of
                              the cursor path
  three clusters              2^25 rows, 40 random bits around three far-apart centres: empty cells, empty and one-tile regions
  other types and modes       uint64; int32 and uint32 at 2^25 + 1; N(0, 1) doubles and round(N(0, 1) * 2^40) int64 in splitter mode
  crowded cells               100 rows per 64-bit id: the cells go to `todo` and k_local_sort
  sorted_order                int64 at 2^25 rows with 2^20 duplicated keys: a permutation, the gathered keys are the oracle's sort, ties in row order
  8-byte-aligned buffers      the column and the output one element into their buffers
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import c_oracle
from oracle import cudf_oracle as orc

N25 = 1 << 25


@pytest.fixture(scope="module")
def gx():
    import torch
    assert torch.cuda.is_available()
    import cudf_amd  # noqa: F401
    from cudf_amd import Column, ops, _lib as L
    yield Column, ops, L


def _sort(gx, v, descending=False, misaligned=False):
    """gx_sort_keys through the C ABI -> (sorted numpy array, cursor-path state, splitter mode on, cells left to k_local_sort).
    misaligned: the column is v[1:] AT ITS PLACE inside v's buffer, the output starts one element into its buffer"""
    Column, ops, L = gx
    col = Column.from_numpy(v)
    out = Column.empty(v.dtype, v.size)
    off, n = (1, v.size - 1) if misaligned else (0, v.size)
    src, dst = col.data.data_ptr(), out.data.data_ptr()
    if misaligned:
        assert src % 16 == 0 and dst % 16 == 0
    isz = v.dtype.itemsize
    tmp = ops._run(L.lib.gx_sort_keys, col.gx, ctypes.c_void_p(src + isz * off), ctypes.c_void_p(dst + isz * off), n, int(descending))
    ops._check_sort_status(tmp)
    st = ctypes.c_int32(-1)
    L.check(L.lib.gx_sort_cursor_state(ops.ptr(tmp), ctypes.byref(st), ops.stream_ptr()), "gx_sort_cursor_state")
    split = (ctypes.c_int32 * 4)()
    L.check(L.lib.gx_sort_split_info(ops.ptr(tmp), split, ops.stream_ptr()), "gx_sort_split_info")
    todo = ctypes.c_int32(-1)
    L.check(L.lib.gx_sort_place_info(ops.ptr(tmp), ctypes.byref(todo), ops.stream_ptr()), "gx_sort_place_info")
    return out.to_numpy()[off:], st.value, int(split[0]), todo.value


def _make(kind, n):
    rng = np.random.default_rng([n, sum(kind.encode())])
    if kind == "i64_full":
        return rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
    if kind == "u64_full":
        return rng.integers(0, 2**64 - 1, n, dtype=np.uint64)
    if kind == "i32_full":
        return rng.integers(-2**31, 2**31 - 1, n, dtype=np.int32)
    if kind == "u32_full":
        return rng.integers(0, 2**32 - 1, n, dtype=np.uint32)
    if kind == "clusters":    # 40 random bits around three far-apart centres
        centre = np.array([-(1 << 62), 1 << 45, (1 << 62) + (1 << 61)], dtype=np.int64)
        return centre[rng.integers(0, 3, n)] + rng.integers(0, 1 << 40, n, dtype=np.int64)
    if kind == "f64_normal":  # N(0, 1) doubles: both signs, no NaN, no zero of either sign
        v = rng.standard_normal(n)
        v[v == 0] = 1.0
        return v
    if kind == "i64_normal":  # bell-shaped around zero
        return np.round(rng.standard_normal(n) * float(1 << 40)).astype(np.int64)
    if kind == "dupids":      # 100 rows per 64-bit id, in random row order
        ids = rng.integers(-2**63, 2**63 - 1, (n + 99) // 100, dtype=np.int64)
        return rng.permutation(np.repeat(ids, 100)[:n])
    if kind == "i64_ties":    # full range, the last 2^20 rows repeat the first 2^20
        v = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
        v[-(1 << 20):] = v[:1 << 20]
        return v
    raise AssertionError(kind)


class _Inputs:
    """(column, ascending oracle result) per (kind, rows): generated and sorted by the oracle once, read-only afterwards; the previous kind
    is dropped when another is asked for (the tests go kind by kind).  Descending expectations of integer keys are the reversed
    ascending result: equal integer keys are bit-identical."""

    def __init__(self):
        self.kind = None
        self.have = {}

    def get(self, kind, n):
        if self.kind != kind:
            self.kind, self.have = kind, {}
        if n not in self.have:
            v = _make(kind, n)
            asc = c_oracle.sort_i64(v) if v.dtype == np.int64 else orc.sort_keys(v)
            for a in (v, asc):
                a.setflags(write=False)
            self.have[n] = (v, asc)
        return self.have[n]


@pytest.fixture(scope="module")
def inputs():
    return _Inputs()


def test_expectation_shortcuts_are_the_oracles_own():
    v = np.random.default_rng(1).integers(-50, 50, 100_000, dtype=np.int64)
    asc = c_oracle.sort_i64(v)
    assert c_oracle.sort_i64(v, descending=True).tobytes() == asc[::-1].tobytes()
    assert c_oracle.sort_i64(v[1:].copy()).tobytes() == np.delete(asc, int(np.searchsorted(asc, v[0]))).tobytes()


# ---- 1. full-range int64: the bit-digit path of level 1 and of the cell kernel
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("n", [N25 + 1, 40_000_003])
def test_full_range_int64(gx, inputs, n, descending):
    v, asc = inputs.get("i64_full", n)
    got, state, split, todo = _sort(gx, v, descending)
    print(f"n={n} i64_full descending={descending}: state {state} split {split} todo {todo}")
    assert got.tobytes() == (asc[::-1] if descending else asc).tobytes()
    assert state == 3 and split == 0, (state, split)


# ---- 8. column and output only 8-byte aligned: level 1's regions start on either parity, cell slots stay aligned
@pytest.mark.parametrize("descending", [False, True])
def test_full_range_int64_from_8_byte_aligned_buffers(gx, inputs, descending):
    v, asc = inputs.get("i64_full", N25 + 1)
    asc1 = np.delete(asc, int(np.searchsorted(asc, v[0])))   # v[1:] sorted: one copy of v[0] taken out
    got, state, split, todo = _sort(gx, v, descending, misaligned=True)
    print(f"n={v.size - 1} i64_full misaligned descending={descending}: state {state} split {split} todo {todo}")
    assert got.tobytes() == (asc1[::-1] if descending else asc1).tobytes()
    assert state == 3 and split == 0, (state, split)


# ---- 2. several cells per workgroup: the entry words hold over the walk and the LDS reuse
@pytest.mark.parametrize("grid", [1000])
def test_a_small_grid_walks_the_cells(gx, inputs, grid):
    _, _, L = gx
    v, asc = inputs.get("i64_full", N25 + 1)
    L.lib.gx_sort_set_place_grid(grid)
    try:
        got, state, split, todo = _sort(gx, v)
    finally:
        L.lib.gx_sort_set_place_grid(0)
    print(f"n={v.size} i64_full place grid {grid}: state {state} split {split} todo {todo}")
    assert got.tobytes() == asc.tobytes()
    assert state == 3 and split == 0, (state, split)


# ---- 3. the look-back chain as the only path: fixed slots, a bounded grid walking the cells
@pytest.mark.parametrize("n", [(1 << 22) + 3, (1 << 23) + 12_345])
def test_look_back_path_only(gx, inputs, n):
    _, _, L = gx
    v, asc = inputs.get("i64_full", n)
    L.lib.gx_sort_set_cursor_path(0, 0.0)
    try:
        got, state, split, todo = _sort(gx, v)
    finally:
        L.lib.gx_sort_set_cursor_path(1, 0.0)
    print(f"n={n} i64_full cursor path off: state {state} split {split} todo {todo}")
    assert got.tobytes() == asc.tobytes()
    assert state == 0 and split == 0, (state, split)


# ---- 4. mostly empty buckets and cells
def test_three_far_apart_clusters(gx, inputs):
    v, asc = inputs.get("clusters", N25)
    got, state, split, todo = _sort(gx, v)
    print(f"n={v.size} clusters: state {state} split {split} todo {todo}")
    assert got.tobytes() == asc.tobytes()   # whichever mode the plan picked


# ---- 5. other key types and modes
def test_full_range_uint64(gx, inputs):
    v, asc = inputs.get("u64_full", N25 + 1)
    got, state, split, todo = _sort(gx, v)
    print(f"n={v.size} u64_full: state {state} split {split} todo {todo}")
    assert got.tobytes() == asc.tobytes()
    assert state == 3 and split == 0, (state, split)


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("kind", ["i32_full", "u32_full"])
def test_32_bit_keys(gx, inputs, kind, descending):
    v, asc = inputs.get(kind, N25 + 1)
    got, state, split, todo = _sort(gx, v, descending)
    print(f"n={v.size} {kind} descending={descending}: state {state} split {split} todo {todo}")
    assert got.tobytes() == (asc[::-1] if descending else asc).tobytes()
    assert split == 0, (state, split)   # splitter mode is for 64-bit keys


def test_doubles_in_splitter_mode(gx, inputs):
    v, asc = inputs.get("f64_normal", N25)
    got, state, split, todo = _sort(gx, v)
    print(f"n={v.size} f64_normal: state {state} split {split} todo {todo}")
    assert got.tobytes() == asc.tobytes()
    assert state == 3 and split == 1, (state, split)


@pytest.mark.parametrize("descending", [False, True])
def test_bell_shaped_int64_in_splitter_mode(gx, inputs, descending):
    v, asc = inputs.get("i64_normal", N25)
    got, state, split, todo = _sort(gx, v, descending)
    print(f"n={v.size} i64_normal descending={descending}: state {state} split {split} todo {todo}")
    assert got.tobytes() == (asc[::-1] if descending else asc).tobytes()
    assert state == 3 and split == 1, (state, split)   # the SPLIT form of the cell kernel


# ---- 6. crowded cells: left to k_local_sort through `todo`
def test_crowded_cells(gx, inputs):
    v, asc = inputs.get("dupids", N25)
    got, state, split, todo = _sort(gx, v)
    print(f"n={v.size} dupids: state {state} split {split} todo {todo}")
    assert got.tobytes() == asc.tobytes()
    assert todo != 0, todo   # a bin of 100 equal keys is beyond the windows: no cell was finished by k_local_place alone


# ---- 7. sorted_order: the word sort runs the same two kernels
@pytest.mark.parametrize("ascending", [True, False])
def test_sorted_order(gx, inputs, ascending):
    Column, ops, _ = gx
    v, asc = inputs.get("i64_ties", N25)
    order = ops.sorted_order(Column.from_numpy(v), ascending).to_numpy()
    assert order.dtype == np.int32 and order.size == v.size
    assert np.bincount(order, minlength=v.size).tobytes() == np.ones(v.size, np.int64).tobytes()   # a permutation of the rows
    got = v[order]
    assert got.tobytes() == (asc if ascending else asc[::-1]).tobytes()
    tie = got[1:] == got[:-1]
    print(f"n={v.size} i64_ties ascending={ascending}: {int(tie.sum())} adjacent ties")
    assert int(tie.sum()) >= 1 << 20
    assert bool((order[1:][tie] > order[:-1][tie]).all())   # equal keys stay in row order
