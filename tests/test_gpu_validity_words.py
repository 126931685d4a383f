"""GPU: one contract over every entry point of the C ABI that WRITES validity words (cudf_amd/csrc/gx_validity.hpp is what their
kernels share): gx_gather, gx_gather2, gx_segmented_shift, gx_segmented_fill_nulls, gx_rolling_window (row and tile kernel),
gx_copy_if_else, gx_concatenate, gx_binary_op, gx_compact_column, gx_bitmask_copy.

For every row count around a word, a wave's 64 rows and the 4096-row tiles, and every source begin bit where the entry point takes
one, with about 20 % nulls in the sources: the output bitmap is ceil(n / 32) words followed by two guard words; the bits below n
equal np.packbits(..., bitorder="little") of the NumPy result, the guard words are untouched, the bits of the last word at and
above n are what the entry point has always left there (TAIL), and the returned null count, where there is one, is n - popcount."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS = (1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 4095, 4097)
BEGIN_BITS = (0, 1, 31, 33)
GUARD = np.array([0xDEADBEEF, 0x12345678], dtype=np.uint32)
PRESET = 0xA5A5A5A5                      # what the output words hold before the call
INT32, INT64 = 3, 4                      # gx dtype codes
OP_SUM, BINOP_ADD = 0, 0

# the bits of the last word at and above n: "zero", or "kept" (the word is merged under a mask: what was there stays)
TAIL = {"gather": "zero", "gather2": "zero", "segmented_shift": "zero", "segmented_fill_nulls": "zero", "rolling_rows": "zero",
        "rolling_tile": "zero", "copy_if_else": "zero", "concatenate": "zero", "binary_op": "zero", "compact_column": "zero",
        "bitmask_copy": "kept"}


@pytest.fixture(scope="module")
def L():
    import torch
    from cudf_amd import _lib
    assert torch.cuda.is_available()
    return _lib


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def nwords(n):
    return (n + 31) // 32


def valid_bits(rng, n):
    return rng.random(n) >= 0.2


def bitmap_at(rng, valid, bit):
    """device words whose bits [bit, bit + n) are `valid`; the bits around them are random"""
    n = len(valid)
    bits = rng.integers(0, 2, nwords(bit + n) * 32).astype(np.uint8)
    bits[bit:bit + n] = valid
    return dev(np.packbits(bits, bitorder="little").view(np.uint32))


def out_bitmap(n, preset=PRESET):
    return dev(np.concatenate([np.full(nwords(n), preset, dtype=np.uint32), GUARD]))


def scratch(L, fn, *args):
    import torch
    nb = ctypes.c_size_t(0)
    assert fn(*args, None, ctypes.byref(nb), stream()) == 0
    tmp = torch.empty(max(int(nb.value), 1), dtype=torch.uint8, device="cuda")
    return tmp, nb


def check(name, n, out_valid, want, nulls=None, preset=PRESET):
    words = host(out_valid, np.uint32)
    assert len(words) == nwords(n) + 2
    assert np.array_equal(words[-2:], GUARD), (name, n, "a word behind the bitmap was written", words[-2:])
    want_words = np.packbits(np.concatenate([want, np.zeros(nwords(n) * 32 - n, dtype=bool)]), bitorder="little").view(np.uint32)
    got_bits = np.unpackbits(words[:-2].view(np.uint8), bitorder="little")
    assert np.array_equal(got_bits[:n], want.astype(np.uint8)), (name, n, np.flatnonzero(got_bits[:n] != want)[:8])
    if n % 32:
        above = ~np.uint32((1 << (n % 32)) - 1)
        tail = {"zero": np.uint32(0), "kept": np.uint32(preset) & above}[TAIL[name]]
        assert (words[-3] & above) == tail, (name, n, hex(int(words[-3])), TAIL[name])
    if TAIL[name] == "zero":
        assert np.array_equal(words[:-2], want_words), (name, n)
    if nulls is not None:
        assert int(host(nulls, np.int64)[0]) == n - int(want.sum()), (name, n, int(host(nulls, np.int64)[0]), n - int(want.sum()))


def null_counter():
    return dev(np.array([-77], dtype=np.int64))


@pytest.mark.parametrize("n", ROWS)
def test_gather(L, n):
    rng = np.random.default_rng(100 + n)
    src_rows = 203
    sv = valid_bits(rng, src_rows)
    m = rng.integers(0, src_rows, n).astype(np.int32)
    m[rng.random(n) < 0.1] = src_rows + 3                                  # out of bounds: null under nullify_oob
    src, out, ov = dev(rng.integers(0, 1 << 30, src_rows).astype(np.int32)), dev(np.zeros(n, np.int32)), out_bitmap(n)
    svw, dm = bitmap_at(rng, sv, 0), dev(m)
    assert L.lib.gx_gather(4, ptr(src), ptr(svw), src_rows, ptr(dm), n, 1, ptr(out), ptr(ov), stream()) == 0
    check("gather", n, ov, (m < src_rows) & sv[np.minimum(m, src_rows - 1)])


@pytest.mark.parametrize("n", ROWS)
def test_gather2(L, n):
    rng = np.random.default_rng(200 + n)
    na, nb = 77, 131
    a, b = dev(rng.integers(0, 99, na).astype(np.int64)), dev(rng.integers(0, 99, nb).astype(np.int64))
    for abit, bbit in zip(BEGIN_BITS, BEGIN_BITS[1:] + BEGIN_BITS[:1]):
        av, bv = valid_bits(rng, na), valid_bits(rng, nb)
        m = rng.integers(0, na + nb, n).astype(np.int32)
        m[rng.random(n) < 0.1] = na + nb + 5                               # outside both sides: null
        both = np.concatenate([av, bv, np.zeros(8, dtype=bool)])
        out, ov, nulls = dev(np.zeros(n, np.int64)), out_bitmap(n), null_counter()
        avw, bvw, dm = bitmap_at(rng, av, abit), bitmap_at(rng, bv, bbit), dev(m)
        assert L.lib.gx_gather2(8, ptr(a), ptr(avw), abit, na, ptr(b), ptr(bvw), bbit, nb, ptr(dm), n, ptr(out), ptr(ov), ptr(nulls),
                                stream()) == 0
        check("gather2", n, ov, both[m], nulls)


def group_labels(rng, n):
    heads = rng.random(n) < 0.15
    heads[0] = True
    return heads, (np.cumsum(heads) - 1).astype(np.int32)


@pytest.mark.parametrize("n", ROWS)
def test_segmented_shift(L, n):
    rng = np.random.default_rng(300 + n)
    _, labels = group_labels(rng, n)
    v = valid_bits(rng, n)
    want = np.zeros(n, dtype=bool)                                         # fill_valid == 0: a row without a source is null
    same = labels[1:] == labels[:-1]
    want[1:][same] = v[:-1][same]
    src, out, ov = dev(rng.integers(0, 99, n).astype(np.int16)), dev(np.zeros(n, np.int16)), out_bitmap(n)
    vw, dl = bitmap_at(rng, v, 0), dev(labels)
    assert L.lib.gx_segmented_shift(2, ptr(src), ptr(vw), ptr(dl), n, 1, 0, 0, ptr(out), ptr(ov), stream()) == 0
    check("segmented_shift", n, ov, want)


@pytest.mark.parametrize("n", ROWS)
def test_segmented_fill_nulls(L, n):
    rng = np.random.default_rng(400 + n)
    heads, labels = group_labels(rng, n)
    v = valid_bits(rng, n)
    want = np.zeros(n, dtype=bool)                                         # PRECEDING: valid once the group has had a valid row
    for i in range(n):
        want[i] = v[i] or (i > 0 and not heads[i] and want[i - 1])
    src, out, ov = dev(rng.integers(0, 99, n).astype(np.int8)), dev(np.zeros(n, np.int8)), out_bitmap(n)
    vw, dh = bitmap_at(rng, v, 0), dev(heads.astype(np.uint8))
    args = (1, ptr(src), ptr(vw), ptr(dh), n, 0, ptr(out), ptr(ov))
    tmp, nb = scratch(L, L.lib.gx_segmented_fill_nulls, *args)
    assert L.lib.gx_segmented_fill_nulls(*args, ptr(tmp), ctypes.byref(nb), stream()) == 0
    check("segmented_fill_nulls", n, ov, want)


@pytest.mark.parametrize("name,preceding,following", [("rolling_rows", 2, 0), ("rolling_tile", 12, 3)])
@pytest.mark.parametrize("n", ROWS)
def test_rolling_window(L, n, name, preceding, following):
    rng = np.random.default_rng(500 + n)
    src = dev(rng.integers(-99, 99, n).astype(np.int32))
    for bit in BEGIN_BITS:
        v = valid_bits(rng, n)
        c = np.concatenate([[0], np.cumsum(v)])                            # valid rows of the window [i - p + 1, i + f], cut at the ends
        lo, hi = np.maximum(np.arange(n) - preceding + 1, 0), np.minimum(np.arange(n) + following + 1, n)
        out, ov, nulls = dev(np.zeros(n, np.int64)), out_bitmap(n), null_counter()
        vw = bitmap_at(rng, v, bit)
        assert L.lib.gx_rolling_window(INT32, ptr(src), ptr(vw), bit, n, preceding, following, None, None, None, None, 1, OP_SUM,
                                       ptr(out), ptr(ov), ptr(nulls), stream()) == 0
        check(name, n, ov, (c[hi] - c[lo]) >= 1, nulls)


@pytest.mark.parametrize("n", ROWS)
def test_copy_if_else(L, n):
    rng = np.random.default_rng(600 + n)
    lhs, rhs = dev(rng.integers(0, 99, n).astype(np.int32)), dev(rng.integers(0, 99, n).astype(np.int32))
    for k, lbit in enumerate(BEGIN_BITS):
        rbit, mbit = BEGIN_BITS[(k + 1) % 4], BEGIN_BITS[(k + 2) % 4]
        lv, rv, mv = valid_bits(rng, n), valid_bits(rng, n), valid_bits(rng, n)
        mask = rng.integers(0, 2, n).astype(np.uint8)
        out, ov, nulls = dev(np.zeros(n, np.int32)), out_bitmap(n), null_counter()
        lw, rw, mw, dm = bitmap_at(rng, lv, lbit), bitmap_at(rng, rv, rbit), bitmap_at(rng, mv, mbit), dev(mask)
        assert L.lib.gx_copy_if_else(4, ptr(lhs), ptr(lw), lbit, None, 0, ptr(rhs), ptr(rw), rbit, None, 0, ptr(dm), ptr(mw), mbit, n,
                                     ptr(out), ptr(ov), ptr(nulls), stream()) == 0
        check("copy_if_else", n, ov, np.where((mask != 0) & mv, lv, rv), nulls)


@pytest.mark.parametrize("n", ROWS)
def test_concatenate(L, n):
    rng = np.random.default_rng(700 + n)
    for k in range(4):
        cuts = np.sort(rng.integers(0, n + 1, 2))
        rows = [int(cuts[0]), int(cuts[1] - cuts[0]), int(n - cuts[1])]
        bits = [BEGIN_BITS[(k + j) % 4] for j in range(3)]
        vs = [valid_bits(rng, r) for r in rows]
        cols = [dev(rng.integers(0, 99, max(r, 1)).astype(np.int64)) for r in rows]
        maps = [bitmap_at(rng, v, b) for v, b in zip(vs, bits)]
        arrs = ((ctypes.c_void_p * 3)(*[c.data_ptr() for c in cols]), (ctypes.c_int64 * 3)(*rows),
                (ctypes.c_void_p * 3)(*[m.data_ptr() for m in maps]), (ctypes.c_int64 * 3)(*bits))
        out, ov, nulls = dev(np.zeros(n, np.int64)), out_bitmap(n), null_counter()
        args = (8, 3, *arrs, ptr(out), ptr(ov), ptr(nulls))
        tmp, nb = scratch(L, L.lib.gx_concatenate, *args)
        assert L.lib.gx_concatenate(*args, ptr(tmp), ctypes.byref(nb), stream()) == 0
        check("concatenate", n, ov, np.concatenate(vs), nulls)


@pytest.mark.parametrize("n", ROWS)
def test_binary_op(L, n):
    rng = np.random.default_rng(800 + n)
    lhs, rhs = dev(rng.integers(0, 99, n).astype(np.int32)), dev(rng.integers(0, 99, n).astype(np.int32))
    for k, lbit in enumerate(BEGIN_BITS):
        rbit = BEGIN_BITS[(k + 1) % 4]
        lv, rv = valid_bits(rng, n), valid_bits(rng, n)
        out, ov, nulls = dev(np.zeros(n, np.int32)), out_bitmap(n), null_counter()
        lw, rw = bitmap_at(rng, lv, lbit), bitmap_at(rng, rv, rbit)
        assert L.lib.gx_binary_op(BINOP_ADD, INT32, ptr(lhs), ptr(lw), lbit, None, 0, INT32, ptr(rhs), ptr(rw), rbit, None, 0, n, INT32,
                                  ptr(out), ptr(ov), ptr(nulls), stream()) == 0
        check("binary_op", n, ov, lv & rv, nulls)


@pytest.mark.parametrize("n", ROWS)
def test_compact_column(L, n):
    """n = the SELECTED rows: the output bitmap is what the contract is about (zeroed by the caller, as gx.h asks)"""
    rng = np.random.default_rng(900 + n)
    n_in = n + n // 2 + 3
    keep = np.zeros(n_in, dtype=bool)
    keep[rng.permutation(n_in)[:n]] = True
    src, mask = dev(rng.integers(0, 99, n_in).astype(np.int32)), dev(keep.astype(np.uint8))
    args = (ptr(mask), None, 0, n_in, None)
    plan, nb = scratch(L, L.lib.gx_select_mask, *args)
    assert L.lib.gx_select_mask(*args, ptr(plan), ctypes.byref(nb), stream()) == 0
    for bit in BEGIN_BITS:
        v = valid_bits(rng, n_in)
        out, ov, nulls = dev(np.zeros(n, np.int32)), out_bitmap(n, preset=0), null_counter()
        vw = bitmap_at(rng, v, bit)
        assert L.lib.gx_compact_column(4, ptr(src), ptr(vw), bit, n_in, ptr(plan), ptr(out), ptr(ov), ptr(nulls), stream()) == 0
        check("compact_column", n, ov, v[keep], nulls, preset=0)


@pytest.mark.parametrize("n", ROWS)
def test_bitmask_copy(L, n):
    rng = np.random.default_rng(1000 + n)
    for bit in BEGIN_BITS:
        v = valid_bits(rng, n)
        ov = out_bitmap(n)
        vw = bitmap_at(rng, v, bit)
        assert L.lib.gx_bitmask_copy(ptr(ov), 0, ptr(vw), bit, n, stream()) == 0
        check("bitmask_copy", n, ov, v)
