"""GPU: level 0 of the cursor-path sort behind ONE launch (gx_sort.hip: k_level0).  Level 0 has three alternative forms -- the bit
digit (hf_scatter_tile<.., 0, 8>, 8192-key tiles) and the two LUT forms of splitter mode (sp_level0_tile<.., 0 / 1>, 7168-key tiles);
the plan on the device picks one and every workgroup of the one launch branches to it.  The grid is sized for the form with more
tiles, each form is told its own tile count, and the workgroups past it return.  What can go wrong: a form that takes its swizzle,
its range seams or its last tile from the grid instead of from its own tile count, or surplus workgroups that do not return.

Every case: bit for bit against the plain-C oracle, with the path pinned through gx_sort_cursor_state / gx_sort_split_info AND the
LUT form the plan picked.  gx_sort_split_info reports splitter mode, not the form, so the form is read where the device keeps it:
SplitPlan::lut_log, at byte SP_LUT_FORM_BYTE of the sort's scratch (the plan is the scratch's first bytes; a static_assert next to
SortPlan in gx_sort.hip holds the same number).  Forms 0 and 1 run sp_level0_tile<.., 0>, form 2 runs sp_level0_tile<.., 1>:
  bell-shaped int64 -> form 0 (linear LUT), lognormal int64 -> form 1 (logarithmic LUT), N(0, 1) doubles, both signs, no NaN -> form 2.

The same inputs are sorted once more from a column and into an output that are only 8-byte aligned (data pointer + 8, n - 1 rows):
the C ABI accepts any 8-byte-aligned pointer, so no load or store of the streaming kernels may assume more.

Sizes: the cursor path starts at 2^25 rows, the smallest shape at which these launches exist.  At every size the splitter form has
8 / 7 of the bit-digit form's tiles -- more than a range's worth (an eighth) of surplus workgroups.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import c_oracle
from oracle import cudf_oracle as orc

HF_TILE = 512 * 16   # keys per tile of the bit-digit form (BT * hf_kpt<KeyT>())
SP_TILE = 512 * 14   # keys per tile of the splitter forms (BT * SP_KPT)
NRANGE = 8           # input ranges of level 0
SAMPLE_STEP = 8 * 64  # below 2^27 rows the sample reads the 64-key chunk at every multiple of 512 rows
SP_LUT_FORM_BYTE = 166812  # offsetof(SortPlan, sp) + offsetof(SplitPlan, lut_log): gx_sort.hip asserts the same constant

N_BIT_ONE = 4096 * HF_TILE + 1                   # 2^25 + 1: a one-row last tile of the bit-digit form
N_SP_ONE = -(-(1 << 25) // SP_TILE) * SP_TILE + 1  # the first k * 7168 + 1 above 2^25: a one-row last tile of the splitter forms
N_ODD = 40_000_003                               # neither: both forms end in a part-filled tile, 4883 against 5581 tiles
SIZES = {"bit_one_row_tail": N_BIT_ONE, "sp_one_row_tail": N_SP_ONE, "odd": N_ODD}


def test_sizes_are_what_they_claim():
    assert N_BIT_ONE % HF_TILE == 1 and N_BIT_ONE % SP_TILE != 1
    assert N_SP_ONE % SP_TILE == 1 and N_SP_ONE % HF_TILE != 1 and N_SP_ONE > 1 << 25
    for n in SIZES.values():
        t_bit, t_sp = -(-n // HF_TILE), -(-n // SP_TILE)
        assert n >= 1 << 25 and t_sp - t_bit > t_bit // NRANGE   # more surplus workgroups than one range has tiles


@pytest.fixture(scope="module")
def gx():
    import torch
    assert torch.cuda.is_available()
    import cudf_amd  # noqa: F401
    from cudf_amd import Column, ops, _lib as L
    yield Column, ops, L


def _sort(gx, v, descending=False, misaligned=False):
    """gx_sort_keys through the C ABI -> (sorted numpy array, cursor-path state, gx_sort_split_info + [the LUT form of the plan]).
    misaligned: the column is v[1:] AT ITS PLACE inside v's buffer, the output starts 8 bytes into its buffer"""
    Column, ops, L = gx
    col = Column.from_numpy(v)
    out = Column.empty(v.dtype, v.size)
    off, n = (1, v.size - 1) if misaligned else (0, v.size)
    src, dst = col.data.data_ptr(), out.data.data_ptr()
    if misaligned:
        assert src % 16 == 0 and dst % 16 == 0   # + 8: 8-byte aligned and no more
    tmp = ops._run(L.lib.gx_sort_keys, col.gx, ctypes.c_void_p(src + 8 * off), ctypes.c_void_p(dst + 8 * off), n, int(descending))
    ops._check_sort_status(tmp)
    st = ctypes.c_int32(-1)
    L.check(L.lib.gx_sort_cursor_state(ops.ptr(tmp), ctypes.byref(st), ops.stream_ptr()), "gx_sort_cursor_state")
    split = (ctypes.c_int32 * 4)()
    L.check(L.lib.gx_sort_split_info(ops.ptr(tmp), split, ops.stream_ptr()), "gx_sort_split_info")
    import torch
    form = int(tmp[SP_LUT_FORM_BYTE:SP_LUT_FORM_BYTE + 4].view(torch.int32).item())   # (meaningful when split[0] == 1)
    return out.to_numpy()[off:], st.value, list(split) + [form]


def _make(kind, n):
    rng = np.random.default_rng([n, sum(kind.encode())])
    if kind == "uniform":
        return rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
    if kind == "normal":      # bell-shaped around zero (tests/test_gpu_sort_splitters.py)
        return np.round(rng.standard_normal(n) * float(1 << 40)).astype(np.int64)
    if kind == "lognormal":   # densities over many octaves (tests/test_gpu_sort_splitters.py)
        return np.round(np.exp(rng.standard_normal(n) * 3.0 + 25.0)).astype(np.int64)
    if kind == "f64_normal":  # N(0, 1) doubles: both signs, no NaN, no zero of either sign
        v = rng.standard_normal(n)
        v[v == 0] = 1.0
        return v
    raise AssertionError(kind)


class _Inputs:
    """one (column, ascending oracle result, the same for the column without its first row) at a time: the cases of one input run
    back to back (parametrised size-major), so every input is generated and sorted by the oracle once.  Descending expectations of
    integer keys are the reversed ascending result: equal integer keys are bit-identical."""

    def __init__(self):
        self.key = None
        self.v = self.asc = self.asc1 = None

    def get(self, kind, size):
        if self.key != (kind, size):
            self.v = self.asc = self.asc1 = None
            v = _make(kind, SIZES[size])
            asc = c_oracle.sort_i64(v) if v.dtype == np.int64 else orc.sort_keys(v)
            # v[1:] sorted = the sorted column with ONE copy of v[0] taken out (any copy: equal keys are bit-identical here)
            asc1 = np.delete(asc, int(np.searchsorted(asc, v[0])))
            for a in (v, asc, asc1):
                a.setflags(write=False)
            self.key, self.v, self.asc, self.asc1 = (kind, size), v, asc, asc1
        return self.v, self.asc, self.asc1


@pytest.fixture(scope="module")
def inputs():
    return _Inputs()


def test_expectation_shortcuts_are_the_oracles_own():
    """the two shortcuts of _Inputs, checked against the oracle on a small column with many ties"""
    v = np.random.default_rng(1).integers(-50, 50, 100_000, dtype=np.int64)
    asc = c_oracle.sort_i64(v)
    assert c_oracle.sort_i64(v, descending=True).tobytes() == asc[::-1].tobytes()
    assert c_oracle.sort_i64(v[1:].copy()).tobytes() == np.delete(asc, int(np.searchsorted(asc, v[0]))).tobytes()


# ---- integer keys: the bit-digit form (uniform: splitters off) and the splitter forms (bell-shaped, lognormal), each from an aligned
# and from an 8-byte-aligned column, ascending and descending
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("kind,split_want,form_want", [("uniform", 0, None), ("normal", 1, 0), ("lognormal", 1, 1)])
@pytest.mark.parametrize("size", list(SIZES))
def test_integer_keys_through_the_one_launch(gx, inputs, size, kind, split_want, form_want, misaligned, descending):
    v, asc, asc1 = inputs.get(kind, size)
    got, state, split = _sort(gx, v, descending, misaligned)
    print(f"{size} n={v.size} {kind} misaligned={misaligned} descending={descending}: state {state} split {split}")
    want = asc1 if misaligned else asc
    assert got.tobytes() == (want[::-1] if descending else want).tobytes()
    assert state == 3, (state, split)             # the cursor path sorted the column: level 0 ran in the form the plan picked
    assert split[0] == split_want, (state, split)
    # which LUT form searched: asserted, not assumed.  (Ascending only: descending keys travel complemented, another density for the
    # plan to fit a LUT to, and whichever form it picks there the ascending cases have covered all three at this size.)
    assert form_want is None or descending or split[4] == form_want, (state, split)


# ---- float64 keys of both signs in splitter mode (K_FTOTAL instantiation of the same kernel), aligned and not: LUT form 2,
# sp_level0_tile<.., 1> -- its own tile count for the swizzle, the range seams and the one-row last tile, surplus workgroups returning
@pytest.mark.parametrize("misaligned", [False, True])
@pytest.mark.parametrize("size", list(SIZES))
def test_doubles_of_both_signs_through_the_one_launch(gx, inputs, size, misaligned):
    v, asc, asc1 = inputs.get("f64_normal", size)
    got, state, split = _sort(gx, v, False, misaligned)
    print(f"{size} n={v.size} f64_normal misaligned={misaligned}: state {state} split {split}")
    assert got.tobytes() == (asc1 if misaligned else asc).tobytes()
    assert state == 3 and split[0] == 1, (state, split)
    assert split[4] == 2, (state, split)


# ---- float64 with one NaN the sample cannot see: level 0 -- whichever form -- finds it and the cursor path declines on the device
@pytest.mark.parametrize("size", list(SIZES))
def test_float64_with_an_unsampled_nan_is_declined_on_the_device(gx, size):
    n = SIZES[size]
    v = np.random.default_rng(11).standard_normal(n)
    v[v == 0] = 1.0
    row = n - 1                      # the last row that no sampled chunk holds: in the last tile or the one before, not in the first
    if row % SAMPLE_STEP < 64:
        row -= row % SAMPLE_STEP + 1
    assert row % SAMPLE_STEP >= 64 and n - row <= SP_TILE
    v[row] = np.nan
    got, state, _ = _sort(gx, v)
    assert got.tobytes() == orc.sort_keys(v).tobytes()
    assert state == 2, state         # accepted by the sample, declined by level 0
