"""GPU: launch ROLES of the sort (gx_sort.hip: Role, role_grid).  Behind a cursor-path sort the look-back chain, the LSD passes and
the rescue pass of the big cells are enqueued as FALLBACKS: the host cannot know whether they will run, so the kernels that walk
their tiles / cells with the grid as stride get a grid bounded by a few workgroups per CU.  On the taken path such a launch finds
nothing to do and returns; when the fallback does run, the bounded grid walks every tile.  This module runs each of those kernels in
BOTH roles -- bit for bit against the plain-C oracle, with the path the device took pinned through gx_sort_cursor_state /
gx_sort_info / gx_sort_big_info -- at sizes where the bounded grids wrap unevenly, and it checks that the rewritten sample loop
(k_hf_sample) still sees every chunk it is meant to read: the first, the last (partial) one and one in the middle.  Float keys
keep the look-back chain in the primary role (it is the only path of a column with a NaN); case 8 pins that such a column is
declined on the device and sorted as the reference sorts it.

Sizes: the cursor path starts at 2^25 rows, the smallest shape at which these launches exist.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import c_oracle
from oracle import cudf_oracle as orc

FALLBACK_WGS_PER_CU = 16  # cudf_amd/csrc/gx_sort.hip: `constexpr int FALLBACK_WGS_PER_CU = 16;` (role_grid, above hybrid_cfg)
HF_TILE = 512 * 16        # keys per k_hf_scatter tile of 64-bit keys (BT * hf_kpt<KeyT>())
EXTRA_TILES = 8 * 256     # the level-1 / rescue grid: ceil(n / HF_TILE) + NRANGE * BINS tail tiles
SAMPLE_STEP = 8 * 64      # below 2^27 rows the sample reads the 64-key chunk at every multiple of 512 rows

N_WHOLE = 1 << 25         # whole tiles
N_ONE = (1 << 25) + 1     # a one-row last tile (and a one-row last sample chunk)


@pytest.fixture(scope="module")
def gx():
    import torch
    assert torch.cuda.is_available()
    import cudf_amd  # noqa: F401
    from cudf_amd import Column, ops, _lib as L
    yield Column, ops, L
    L.lib.gx_sort_set_cursor_path(1, 0.0)
    L.lib.gx_sort_set_splitters(1)


def _fallback_grid():
    import torch
    return FALLBACK_WGS_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count


def _n_uneven():
    """the smallest n above 2^25 whose rescue-pass tile count is one more than a multiple of the fallback-role grid, with a one-row
    last tile: the walk's last round holds ONE tile.  (The cell count of the look-back chain is 256 << bits2, a power of two: on a
    grid of 16 x 256 workgroups it cannot be one more than a multiple -- 8192 cells are two even rounds; on a CU count that is not
    a power of two it wraps unevenly as it is.  At 2^25 rows the rescue pass walks 6144 tiles: one round and a half.)"""
    g = _fallback_grid()
    tiles = (N_ONE // HF_TILE) + 2   # (past N_ONE)
    while (tiles + EXTRA_TILES) % g != 1:
        tiles += 1
    return (tiles - 1) * HF_TILE + 1


SIZES = ["whole", "one_row_tail", "uneven_wrap"]


def _size(name):
    return {"whole": N_WHOLE, "one_row_tail": N_ONE, "uneven_wrap": _n_uneven()}[name]


def _sort_with_state(gx, v, descending=False):
    """gx_sort_keys through the C ABI, returning (sorted numpy array, cursor-path state, gx_sort_info, gx_sort_big_info)"""
    Column, ops, L = gx
    col = Column.from_numpy(v)
    out = Column.empty(v.dtype, v.size)
    tmp = ops._run(L.lib.gx_sort_keys, col.gx, col.data_ptr, out.data_ptr, col.size, int(descending))
    ops._check_sort_status(tmp)
    st = ctypes.c_int32(-1)
    L.check(L.lib.gx_sort_cursor_state(ops.ptr(tmp), ctypes.byref(st), ops.stream_ptr()), "gx_sort_cursor_state")
    info = (ctypes.c_int32 * 8)()
    L.check(L.lib.gx_sort_info(ops.ptr(tmp), info, ops.stream_ptr()), "gx_sort_info")
    big = (ctypes.c_int64 * 3)()
    L.check(L.lib.gx_sort_big_info(ops.ptr(tmp), big, ops.stream_ptr()), "gx_sort_big_info")
    split = (ctypes.c_int32 * 4)()
    L.check(L.lib.gx_sort_split_info(ops.ptr(tmp), split, ops.stream_ptr()), "gx_sort_split_info")
    return out.to_numpy(), st.value, list(info), list(big), list(split)


def _make(kind, n):
    rng = np.random.default_rng([n, sum(kind.encode())])
    if kind == "uniform":
        return rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
    if kind == "hot":       # 30 % of the rows carry one key: its cell outgrows every slot
        v = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
        v[rng.random(n) < 0.3] = v[12345]
        return v
    if kind == "int32_skewed":  # keys that agree on everything the two partition levels look at (test_skewed_cells_fall_back_to_lsd)
        return ((rng.integers(0, 2**20, n, dtype=np.int64)) | (1 << 28) | (rng.integers(0, 2, n, dtype=np.int64) << 30)).astype(np.int32)
    raise AssertionError(kind)


class _Inputs:
    """one (column, ascending oracle result) at a time: the cases of one input run back to back (parametrised size-major), so every
    input is generated and sorted by the oracle ONCE.  Descending expectations are the reversed ascending result: equal integer
    keys are bit-identical, so the oracle's descending output is exactly that."""

    def __init__(self):
        self.key = None
        self.v = self.asc = None

    def get(self, kind, size):
        if self.key != (kind, size):
            self.v = self.asc = None
            v = _make(kind, _size(size))
            asc = c_oracle.sort_i64(v) if v.dtype == np.int64 else c_oracle.sort_32(v)
            v.setflags(write=False)
            asc.setflags(write=False)
            self.key, self.v, self.asc = (kind, size), v, asc
        return self.v, self.asc


@pytest.fixture(scope="module")
def inputs():
    return _Inputs()


def _expect(asc, descending):
    return (asc[::-1] if descending else asc).tobytes()


def test_descending_expectation_is_the_oracles_own():
    """the shortcut of _Inputs, checked against the oracle on a small column with many ties"""
    v = np.random.default_rng(1).integers(-50, 50, 100_000, dtype=np.int64)
    assert c_oracle.sort_i64(v, descending=True).tobytes() == c_oracle.sort_i64(v)[::-1].tobytes()


# ---- cases 1-3: one uniform column per size, sorted by the cursor path (primary roles), by the look-back chain as the cursor
# path's FALLBACK (bounded grids) and by the look-back chain as the primary path (cursor path off: full grids)
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("role,state_want", [("primary", 3), ("fallback", 2), ("cursor_off", 0)])
@pytest.mark.parametrize("size", SIZES)
def test_uniform_keys_in_every_role(gx, inputs, size, role, state_want, descending):
    Column, ops, L = gx
    v, asc = inputs.get("uniform", size)
    if role == "fallback":
        L.lib.gx_sort_set_cursor_path(1, -8.0)   # TEST HOOK: every level-0 slot smaller than its estimate -> overflow -> fallback
    elif role == "cursor_off":
        L.lib.gx_sort_set_cursor_path(0, 0.0)
    try:
        got, state, info, big, _ = _sort_with_state(gx, v, descending)
    finally:
        L.lib.gx_sort_set_cursor_path(1, 0.0)
    print(f"{size} n={v.size} {role} descending={descending}: state {state} info {info}")
    assert got.tobytes() == _expect(asc, descending)
    assert state == state_want, (state, info)
    assert info[0] == 1 and info[1] == 1, info    # the hybrid plan was attempted and accepted: the cells were sorted in LDS, no LSD passes
    assert info[7] <= 0, info                       # (k_plan never counted an active LSD pass)


# ---- case 4: a hot value -- the looped rescue pass, the X-mode LSD passes, k_big_distribute
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_hot_value_is_rescued_through_the_looped_pass(gx, inputs, size, descending):
    Column, ops, L = gx
    v, asc = inputs.get("hot", size)
    copies = int((v == v[12345]).sum())
    L.lib.gx_sort_set_splitters(0)   # the bit-digit levels and their big-cell machinery, as tests/test_gpu_sort_big_cells.py
    try:
        got, state, info, big, _ = _sort_with_state(gx, v, descending)
    finally:
        L.lib.gx_sort_set_splitters(1)
    print(f"{size} n={v.size} descending={descending}: state {state} big {big} info {info}")
    assert got.tobytes() == _expect(asc, descending)
    assert state == 3
    assert big[0] == 1 and big[1] == 1                    # ONE big cell, sorted through X
    assert copies <= big[2] <= copies + 3 * 8192          # X = the copies + the cell's ordinary keys
    assert info[1] == 1


# ---- case 5: bell-shaped keys -- splitter mode: k_sp_level0, k_sp_fill
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_bell_shaped_keys_take_the_splitter_mode(gx, size, descending):
    n = _size(size)
    v = np.round(np.random.default_rng(5).standard_normal(n) * float(1 << 40)).astype(np.int64)
    got, state, info, _, split = _sort_with_state(gx, v, descending)
    print(f"{size} n={n} descending={descending}: state {state} split {split} info {info}")
    assert got.tobytes() == c_oracle.sort_i64(v, descending=descending).tobytes()
    assert state == 3 and split[0] == 1, (state, split)


# ---- case 6: int32 keys with skewed cells -- the LSD passes are the only fallback
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_int32_skewed_cells_fall_back_to_the_lsd_passes(gx, inputs, size, descending):
    v, asc = inputs.get("int32_skewed", size)
    got, state, info, _, _ = _sort_with_state(gx, v, descending)
    print(f"{size} n={v.size} descending={descending}: state {state} info {info}")
    assert got.tobytes() == _expect(asc, descending)
    assert info[1] == 0 and info[7] > 0, info             # hybrid not ok; LSD passes active


# ---- case 7: a narrow range -- the counting sort
@pytest.mark.parametrize("size", SIZES)
def test_narrow_range_is_counted(gx, size):
    n = _size(size)
    v = np.random.default_rng(10).integers(100, 10001, n, dtype=np.int64)
    asc = c_oracle.sort_i64(v)
    for descending in (False, True):
        got, state, _, _, _ = _sort_with_state(gx, v, descending)
        assert got.tobytes() == _expect(asc, descending)
        assert state == 5, state


# ---- case 8: float64 with one NaN the sample cannot see -- level 0 finds it and the cursor path declines on the device; the stable
# look-back chain sorts the column.  For float keys that chain is the only path of such a column and stays in the PRIMARY role.
# (One direction per size: the reference's stable argsort of the floats takes longer than everything else in this module.)
@pytest.mark.parametrize("size", SIZES)
def test_float64_with_an_unsampled_nan_is_declined_on_the_device(gx, size):
    n = _size(size)
    v = np.random.default_rng(11).standard_normal(n)
    v[v == 0] = 1.0
    v[64 + 5] = np.nan               # the sample takes rows [c * 512, c * 512 + 64): row 69 is in no sampled chunk
    assert (64 + 5) % SAMPLE_STEP >= 64
    got, state, _, _, _ = _sort_with_state(gx, v)
    assert got.tobytes() == orc.sort_keys(v).tobytes()
    assert state == 2, state         # accepted by the sample, declined by level 0


# ---- case 9: sample coverage -- ONE key with a higher top bit than the rest INSIDE a sampled chunk: the sample's digit positions
# are the column's and the plan is accepted (state 3).  A sample loop that dropped the chunk would plan for bit 61 and level 0 would
# reject it (state 2: tests/test_gpu_sort_cursor_path.py covers a key outside every chunk).  The last sampled chunk is partial at
# two of the three sizes (one row); at 2^25 rows it is whole.
@pytest.mark.parametrize("where", ["first_chunk", "last_chunk", "middle_chunk"])
@pytest.mark.parametrize("size", SIZES)
def test_sample_reads_the_chunk(gx, size, where):
    n = _size(size)
    nchunks = -(-n // SAMPLE_STEP)
    last0 = (nchunks - 1) * SAMPLE_STEP
    assert size == "whole" or n - last0 == 1      # the last sampled chunk holds one row
    row = {"first_chunk": 5, "last_chunk": min(n - 1, last0 + 63), "middle_chunk": (nchunks // 2) * SAMPLE_STEP + 17}[where]
    assert row % SAMPLE_STEP < 64 and row < n
    v = np.random.default_rng(9).integers(0, 2**62, n, dtype=np.int64)
    v[row] = 2**62 + 12345
    got, state, info, _, _ = _sort_with_state(gx, v)
    print(f"{size} {where} row {row} of {n}: state {state} info {info}")
    assert got.tobytes() == c_oracle.sort_i64(v).tobytes()
    assert state == 3, (state, info)
