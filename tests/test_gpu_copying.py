"""GPU: cudf::concatenate / scatter / copy_if_else -- ops.concatenate, ops.scatter, ops.copy_if_else, cudf_amd.concat,
DataFrame.where / mask and the three entry points under them (cudf_amd/csrc/gx_copying.hip), plus the C++ surface with slice and
split (tests/cpp/cudf_copying_tests).  The reference is NumPy: np.concatenate of values and of unpacked validity, out[map] = src
on a copy of the target, np.where.  Everything is compared bit-exactly: values through their unsigned integer views (NaN payloads
and -0.0 count), validity bit by bit, null counts as integers.  Row counts come from gx_concat_tile_rows() = T."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ["int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float32", "float64", "bool"]
BEGIN_BITS = (0, 1, 31, 33)
BIG = 2**22 + 4097


@pytest.fixture(scope="module")
def gx():
    import cudf_amd
    from cudf_amd import Column, ops
    return cudf_amd, Column, ops


@pytest.fixture(scope="module")
def T(gx):
    return int(gx[0]._lib.lib.gx_concat_tile_rows())


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def values(rng, dt, n):
    """n values of dt that use the whole width; floats carry NaNs with payloads, infinities and both zeros"""
    dt = np.dtype(dt)
    if dt == np.bool_:
        return rng.integers(0, 2, n).astype(np.bool_)
    if dt.kind == "f":
        u = {4: np.uint32, 8: np.uint64}[dt.itemsize]
        raw = rng.integers(0, np.iinfo(u).max, n, dtype=u, endpoint=True)
        special = np.array([0, 1 << (dt.itemsize * 8 - 1)], dtype=u)          # +0.0, -0.0
        pick = rng.random(n) < 0.1
        raw[pick] = special[rng.integers(0, 2, int(pick.sum()))]
        return raw.view(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)


def make(gx, rng, dt, n, nullable, p_valid=0.7):
    """(Column, values, validity as bool array -- all true without a mask)"""
    _, Column, _ = gx
    v = values(rng, dt, n)
    valid = rng.random(n) < p_valid if nullable else None
    return Column.from_numpy(v, valid), v, (valid if nullable else np.ones(n, dtype=bool))


def check_column(got, want_values, want_valid, what=""):
    """bit-exact values, validity and null count; a column without nulls must come back without a mask"""
    assert got.size == len(want_values), what
    assert got.dtype == want_values.dtype, what
    assert np.array_equal(bits_of(got.to_numpy()), bits_of(want_values)), what
    nulls = int((~want_valid).sum())
    assert got.null_count == nulls, (what, got.null_count, nulls)
    if nulls == 0:
        assert got.mask is None, what
    else:
        assert got.mask is not None and np.array_equal(got.valid_numpy(), want_valid), what


def check_concat(gx, parts, what=""):
    _, _, ops = gx
    got = ops.concatenate([p[0] for p in parts])
    check_column(got, np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]), what)


# ------------------------------------------------------------------------------------------------ concatenate
@pytest.fixture(scope="module")
def pool(gx, T):
    """one nullable int64 input per length, made once and shared (concatenate does not write its inputs)"""
    rng = np.random.default_rng(11)
    return {n: make(gx, rng, "int64", n, True) for n in (0, 1, 31, 32, 33, 63, 64, 65, T - 1, T, T + 1)}


def test_concatenate_all_ordered_pairs_of_lengths(gx, pool):
    for a, b in itertools.product(pool, repeat=2):
        check_concat(gx, [pool[a], pool[b]], (a, b))


def test_concatenate_triples_with_an_empty_input_in_the_middle(gx, pool):
    for a, b in itertools.product(pool, repeat=2):
        check_concat(gx, [pool[a], pool[0], pool[b]], (a, 0, b))
    check_concat(gx, [pool[0], pool[0], pool[33]], "two empty inputs in front")
    check_concat(gx, [pool[33], pool[0], pool[0]], "two empty inputs at the end")


@pytest.mark.parametrize("dt", ["int8", "int16", "int32", "int64"])
def test_concatenate_misaligned_destinations(gx, T, dt):
    """odd row counts in front: the destination of every later input is misaligned against its source, for 1- and 2-byte types
    not even 4-byte aligned"""
    rng = np.random.default_rng(12)
    for lens in ((1, T + 5, 3, 2 * T + 1, 7), (3, 5, T, 1, T - 1), (7, 64, 9, 4 * T + 2), (2, 2 * T + 3, 6, 65), (5, 1, 1, 1, T + 9)):
        check_concat(gx, [make(gx, rng, dt, n, n % 2 == 1) for n in lens], (dt, lens))


@pytest.mark.parametrize("dt", DTYPES)
def test_concatenate_every_dtype(gx, T, dt):
    rng = np.random.default_rng(13)
    check_concat(gx, [make(gx, rng, dt, n, True) for n in (33, 0, T + 1, 65)], dt)


@pytest.mark.parametrize("count", [1, 17])
def test_concatenate_input_counts(gx, T, count):
    rng = np.random.default_rng(14)
    lens = [int(x) for x in rng.integers(0, T // 2, count)]
    parts = [make(gx, rng, "int32", n, k % 3 != 0) for k, n in enumerate(lens)]
    check_concat(gx, parts, lens)
    if count == 1:                                         # one input: a copy that shares no storage
        got = gx[2].concatenate([parts[0][0]])
        assert got.data.data_ptr() != parts[0][0].data.data_ptr()


def test_concatenate_1025_small_inputs(gx):
    """1 ... 3 rows each: every output word is fed by 11 to 32 inputs, every tile takes the row path"""
    rng = np.random.default_rng(15)
    for dt in ("int64", "int8"):
        parts = [make(gx, rng, dt, int(n), True) for n in rng.integers(1, 4, 1025)]
        check_concat(gx, parts, dt)
    ones = [make(gx, rng, "int16", 1, True, 0.5) for _ in range(1025)]
    check_concat(gx, ones, "32 inputs per word")


def test_concatenate_nullability_mixes(gx, T):
    _, Column, ops = gx
    rng = np.random.default_rng(16)
    lens = (T - 3, 37, T + 2)
    for mix in itertools.product((False, True), repeat=3):
        parts = [make(gx, rng, "float64", n, nb) for n, nb in zip(lens, mix)]
        check_concat(gx, parts, mix)
        if not any(mix):
            assert ops.concatenate([p[0] for p in parts]).mask is None
    v = values(rng, "int32", 70)
    all_null = (Column.from_numpy(v, np.zeros(70, dtype=bool)), v, np.zeros(70, dtype=bool))
    check_concat(gx, [make(gx, rng, "int32", 45, False), all_null, make(gx, rng, "int32", 45, True)], "an all-null input")
    # a mask without nulls counts as no mask
    clean = Column.from_numpy(v, np.ones(70, dtype=bool))
    assert ops.concatenate([clean, clean]).mask is None


def shifted_mask(rng, valid, begin_bit):
    """device words that hold `valid` from begin_bit on, noise in front of and behind it"""
    import torch
    bits = rng.integers(0, 2, begin_bit + len(valid) + 40).astype(np.uint8)
    bits[begin_bit:begin_bit + len(valid)] = valid
    pad = np.zeros((len(bits) + 511) // 512 * 512, dtype=np.uint8)
    pad[:len(bits)] = bits
    return torch.from_numpy(np.packbits(pad, bitorder="little").view(np.int32).copy()).cuda()


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda() if a.size else torch.empty(1, dtype=torch.uint8, device="cuda")


def unpack(words, n):
    return np.unpackbits(words.cpu().numpy().view(np.uint8), bitorder="little")[:n].astype(bool)


def test_concatenate_raw_abi_begin_bits_and_null_count(gx, T):
    """what a sliced view hands down: bitmaps read from begin bits 0 / 1 / 31 / 33, chosen independently for three inputs (one of
    them without a bitmap); the null count is counted by the kernel"""
    import torch
    lib = gx[0]._lib.lib
    rng = np.random.default_rng(17)
    for trial, bbits in enumerate(itertools.product(BEGIN_BITS, repeat=3)):
        lens = (33 + trial, T - 1, 70)
        vals = [values(rng, "int16", n) for n in lens]
        valid = [rng.random(n) < 0.6 for n in lens]
        valid[1 + trial % 2] = None                        # one input without a bitmap
        data = [dev(v) for v in vals]
        masks = [shifted_mask(rng, m, b) if m is not None else None for m, b in zip(valid, bbits)]
        n = sum(lens)
        out = torch.empty(n * 2, dtype=torch.uint8, device="cuda")
        out_valid = torch.full(((n + 511) // 512 * 16,), 0x55555555, dtype=torch.int32, device="cuda")
        nulls = torch.full((1,), -7, dtype=torch.int64, device="cuda")
        k = 3
        ptrs = (ctypes.c_void_p * k)(*[d.data_ptr() for d in data])
        rows = (ctypes.c_int64 * k)(*lens)
        vp = (ctypes.c_void_p * k)(*[m.data_ptr() if m is not None else None for m in masks])
        bb = (ctypes.c_int64 * k)(*bbits)
        nb = ctypes.c_size_t(0)
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.gx_concatenate(2, k, ptrs, rows, vp, bb, None, None, None, None, ctypes.byref(nb), s) == 0
        tmp = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
        assert lib.gx_concatenate(2, k, ptrs, rows, vp, bb, out.data_ptr(), out_valid.data_ptr(), nulls.data_ptr(), tmp.data_ptr(),
                                  ctypes.byref(nb), s) == 0
        want_valid = np.concatenate([m if m is not None else np.ones(ln, dtype=bool) for m, ln in zip(valid, lens)])
        assert np.array_equal(out.cpu().numpy().view(np.int16), np.concatenate(vals)), bbits
        assert np.array_equal(unpack(out_valid, n), want_valid), bbits
        assert not unpack(out_valid, (n + 31) // 32 * 32)[n:].any(), "bits behind the last row are 0"
        assert int(nulls.item()) == int((~want_valid).sum()), bbits


def test_concatenate_large_from_five_uneven_inputs(gx):
    rng = np.random.default_rng(18)
    lens = (1, 2**21 + 77, 4097 - 77 - 1 - 333, 333, 2**21)
    assert sum(lens) == BIG
    check_concat(gx, [make(gx, rng, "int64", n, k != 3) for k, n in enumerate(lens)], "2^22 + 4097 rows")


def test_concatenate_tables_three_columns_of_mixed_width(gx, T):
    _, _, ops = gx
    rng = np.random.default_rng(19)
    lens = (T + 3, 0, 129, 1)
    tables = [[make(gx, rng, dt, n, nb) for dt, nb in (("int8", True), ("float64", False), ("uint16", True))] for n in lens]
    got = ops.concatenate_tables([[c[0] for c in t] for t in tables])
    assert len(got) == 3
    for k in range(3):
        check_column(got[k], np.concatenate([t[k][1] for t in tables]), np.concatenate([t[k][2] for t in tables]), k)


# ------------------------------------------------------------------------------------------------ scatter
SRC_ROWS = (0, 1, 63, 64, 65, 4097)
TGT_ROWS = (1, 64, 65, 2**20 + 3)


@pytest.fixture(scope="module")
def targets(gx):
    """(Column, values, validity) per (rows, nullable), made once: scatter writes a copy"""
    rng = np.random.default_rng(21)
    return {(n, nb): make(gx, rng, "int64", n, nb, 0.8) for n in TGT_ROWS for nb in (False, True)}


def maps_for(rng, ns, nt):
    """(name, map) of ns entries into nt target rows, each target row hit at most once"""
    inj = rng.permutation(nt)[:ns].astype(np.int32)
    rev = (nt - 1 - np.arange(ns)).astype(np.int32)
    neg = (np.arange(ns) - nt).astype(np.int32)            # i - n: row i counted from the end
    return (("random injective", inj), ("reversed", rev), ("negative", neg))


def check_scatter(gx, src, smap, tgt, what):
    _, Column, ops = gx
    got = ops.scatter([src[0]], Column.from_numpy(smap), [tgt[0]])[0]
    want_v, want_ok = tgt[1].copy(), tgt[2].copy()
    want_v[smap] = src[1][:len(smap)]
    want_ok[smap] = src[2][:len(smap)]
    check_column(got, want_v, want_ok, what)
    assert got.data.data_ptr() != tgt[0].data.data_ptr()


@pytest.mark.parametrize("nt", TGT_ROWS)
def test_scatter_rows_maps_and_nullability(gx, targets, nt):
    rng = np.random.default_rng(22 + nt % 7)
    for ns in SRC_ROWS:
        if ns > nt:
            continue
        for src_nullable, tgt_nullable in itertools.product((False, True), repeat=2):
            src = make(gx, rng, "int64", ns, src_nullable, 0.5)
            for name, smap in maps_for(rng, ns, nt):
                check_scatter(gx, src, smap, targets[(nt, tgt_nullable)], (ns, nt, src_nullable, tgt_nullable, name))
    # the untouched target is still what it was
    for nb in (False, True):
        c, v, ok = targets[(nt, nb)]
        assert np.array_equal(c.to_numpy(), v) and (not nb or np.array_equal(c.valid_numpy(), ok))


@pytest.mark.parametrize("n", [64, 65, 2**20 + 3])
def test_scatter_full_reversed_permutation(gx, targets, n):
    """every target row is written: each validity word takes 32 atomic updates, from waves far apart"""
    rng = np.random.default_rng(23)
    smap = (n - 1 - np.arange(n)).astype(np.int32)
    for src_nullable, tgt_nullable in itertools.product((False, True), repeat=2):
        src = make(gx, rng, "int64", n, src_nullable, 0.5)
        check_scatter(gx, src, smap, targets[(n, tgt_nullable)], (n, src_nullable, tgt_nullable))


@pytest.mark.parametrize("dt", DTYPES)
def test_scatter_every_dtype(gx, dt):
    rng = np.random.default_rng(24)
    src, tgt = make(gx, rng, dt, 300, True, 0.5), make(gx, rng, dt, 1000, True, 0.8)
    check_scatter(gx, src, rng.permutation(1000)[:300].astype(np.int32), tgt, dt)


def test_scatter_a_shorter_map_than_the_source(gx):
    rng = np.random.default_rng(25)
    src, tgt = make(gx, rng, "int32", 100, True), make(gx, rng, "int32", 80, False)
    check_scatter(gx, src, rng.permutation(80)[:37].astype(np.int32), tgt, "37 of 100 source rows")


def test_scatter_scalars_valid_and_invalid_two_columns(gx):
    _, Column, ops = gx
    rng = np.random.default_rng(26)
    for n, k in ((1, 1), (65, 64), (4097, 1000), (2**20 + 3, 4097)):
        a, b = make(gx, rng, "int64", n, False), make(gx, rng, "float32", n, True, 0.8)
        idx = rng.permutation(n)[:k].astype(np.int32)
        idx[::2] -= n                                       # every other index counted from the end
        for va, vb in ((True, True), (True, False), (False, True), (False, False)):
            got = ops.scatter_scalar([-(2**40) - 5, 2.5], [va, vb], Column.from_numpy(idx), [a[0], b[0]])
            for g, (c, v, ok), val, valid in ((got[0], a, -(2**40) - 5, va), (got[1], b, 2.5, vb)):
                want_v, want_ok = v.copy(), ok.copy()
                want_v[idx] = val
                want_ok[idx] = valid
                check_column(g, want_v, want_ok, (n, k, va, vb))
    got = ops.scatter_scalar([7, None], None, Column.from_numpy(np.array([0], dtype=np.int32)), [a[0], b[0]])
    assert got[0].to_numpy()[0] == 7 and got[1].null_count == b[0].null_count + int(b[2][0])


def test_scatter_a_map_that_repeats_target_rows(gx):
    """every written row holds one of its candidate (value, validity) pairs -- value AND validity from one source row -- and the rest
    is untouched.  Candidates of one target row differ in value and in validity."""
    _, Column, ops = gx
    rng = np.random.default_rng(27)
    for ns, nt in ((4097, 64), (2**18, 1000), (2**18, 2**18)):
        src_v = np.arange(ns, dtype=np.int64) * 3 + 1       # distinct values: a value names its source row
        src_ok = rng.random(ns) < 0.5
        tgt = make(gx, rng, "int64", nt, True, 0.8)
        tgt_v = -np.arange(nt, dtype=np.int64) - 1           # negative: never a source value
        tgt_c = Column.from_numpy(tgt_v, tgt[2])
        smap = rng.integers(0, nt // 2, ns).astype(np.int32)     # the upper half stays untouched
        smap[::3] -= nt
        got = ops.scatter([Column.from_numpy(src_v, src_ok)], Column.from_numpy(smap), [tgt_c])[0]
        gv = got.to_numpy()
        gok = got.valid_numpy() if got.mask is not None else np.ones(nt, dtype=bool)
        rows = np.where(smap < 0, smap + nt, smap)
        hit = np.zeros(nt, dtype=bool)
        hit[rows] = True
        assert np.array_equal(gv[~hit], tgt_v[~hit]) and np.array_equal(gok[~hit], tgt[2][~hit])
        winner = (gv[hit] - 1) // 3                          # the source row whose value the target holds
        assert np.all((gv[hit] - 1) % 3 == 0) and np.all((winner >= 0) & (winner < ns))
        assert np.array_equal(rows[winner], np.flatnonzero(hit)), "the value came from a row mapped here"
        assert np.array_equal(gok[hit], src_ok[winner]), "value and validity come from the same candidate"
        assert got.null_count == int((~gok).sum())


# ------------------------------------------------------------------------------------------------ copy_if_else
def check_select(gx, lhs, rhs, mask, what):
    """lhs / rhs: (Column, values, validity) or (python scalar or None, dtype); mask: (Column, values, validity)"""
    _, _, ops = gx
    n = mask[0].size

    def side(s):
        if len(s) == 3:
            return s[0], s[1], s[2]
        val, dt = s
        v = np.zeros(n, dtype=dt)
        if val is not None:
            v[:] = val
        return val, v, np.full(n, val is not None)

    (la, lv, lok), (ra, rv, rok) = side(lhs), side(rhs)
    pick = mask[1].astype(bool) & mask[2]
    got = ops.copy_if_else(la, ra, mask[0])
    want_ok = np.where(pick, lok, rok)
    want_bits = np.where(pick, bits_of(lv), bits_of(rv))
    assert got.size == n and got.dtype == lv.dtype, what
    g = bits_of(got.to_numpy())
    # an invalid scalar's value is not specified: compare values where the result is valid, all of them when no scalar is invalid
    cmp = np.ones(n, dtype=bool) if (la is not None and ra is not None) else want_ok
    assert np.array_equal(g[cmp], want_bits[cmp]), what
    nulls = int((~want_ok).sum())
    assert got.null_count == nulls, (what, got.null_count, nulls)
    if nulls == 0:
        assert got.mask is None, what
    else:
        assert np.array_equal(got.valid_numpy(), want_ok), what


def make_mask(gx, rng, n, kind, nullable):
    _, Column, _ = gx
    v = {"true": np.ones(n, dtype=bool), "false": np.zeros(n, dtype=bool), "random": rng.random(n) < 0.5}[kind]
    ok = rng.random(n) < 0.8 if nullable else None
    return Column.from_numpy(v, ok), v, (ok if nullable else np.ones(n, dtype=bool))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4095, 4096, 4097])
def test_copy_if_else_rows_masks_and_nullability(gx, n):
    rng = np.random.default_rng(31 + n)
    for kind, mask_nullable in itertools.product(("true", "false", "random"), (False, True)):
        mask = make_mask(gx, rng, n, kind, mask_nullable)
        for ln, rn in itertools.product((False, True), repeat=2):
            check_select(gx, make(gx, rng, "int64", n, ln), make(gx, rng, "int64", n, rn), mask, (n, kind, mask_nullable, ln, rn))


def test_copy_if_else_large(gx):
    rng = np.random.default_rng(32)
    mask = make_mask(gx, rng, BIG, "random", True)
    check_select(gx, make(gx, rng, "int64", BIG, True), make(gx, rng, "int64", BIG, False), mask, "2^22 + 4097 rows")
    check_select(gx, make(gx, rng, "int8", BIG, False), make(gx, rng, "int8", BIG, False), make_mask(gx, rng, BIG, "random", False), "no bitmaps")


def test_copy_if_else_columns_and_scalars_nine_combinations(gx):
    rng = np.random.default_rng(33)
    n = 4097
    for dt, val in (("int64", -(2**50) + 3), ("float32", -0.0), ("uint8", 200)):
        mask = make_mask(gx, rng, n, "random", True)
        for lk, rk in itertools.product(("column", "valid", "invalid"), repeat=2):
            if lk == rk == "invalid":
                continue   # two invalid scalars carry no type on the Python surface: test_copy_if_else_two_invalid_scalars_through_the_abi
            mk = {"column": lambda: make(gx, rng, dt, n, True), "valid": lambda: (np.dtype(dt).type(val), dt), "invalid": lambda: (None, dt)}
            check_select(gx, mk[lk](), mk[rk](), mask, (dt, lk, rk))


def test_copy_if_else_two_invalid_scalars_through_the_abi(gx):
    """the ninth combination: both sides invalid scalars -- every row null, whatever the mask"""
    import torch
    lib = gx[0]._lib.lib
    n = 4097
    rng = np.random.default_rng(34)
    val = torch.zeros(8, dtype=torch.uint8, device="cuda")
    bad = torch.zeros(1, dtype=torch.uint8, device="cuda")
    mask = dev(rng.random(n) < 0.5)
    out = torch.empty(n * 8, dtype=torch.uint8, device="cuda")
    out_valid = torch.full(((n + 511) // 512 * 16,), -1, dtype=torch.int32, device="cuda")
    nulls = torch.zeros(1, dtype=torch.int64, device="cuda")
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.gx_copy_if_else(8, val.data_ptr(), None, 0, bad.data_ptr(), 1, val.data_ptr(), None, 0, bad.data_ptr(), 1, mask.data_ptr(), None, 0,
                               n, out.data_ptr(), out_valid.data_ptr(), nulls.data_ptr(), s) == 0
    assert int(nulls.item()) == n and not unpack(out_valid, n).any()


@pytest.mark.parametrize("dt", DTYPES)
def test_copy_if_else_every_dtype(gx, dt):
    rng = np.random.default_rng(35)
    n = 1000
    check_select(gx, make(gx, rng, dt, n, True), make(gx, rng, dt, n, True), make_mask(gx, rng, n, "random", True), dt)


def test_copy_if_else_raw_abi_begin_bits(gx):
    """the three bitmaps read from begin bits chosen independently from 0 / 1 / 31 / 33; the null count is counted by the kernel"""
    import torch
    lib = gx[0]._lib.lib
    rng = np.random.default_rng(36)
    n = 4097 + 64
    lv, rv = values(rng, "int32", n), values(rng, "int32", n)
    mv = rng.random(n) < 0.5
    lok, rok, mok = (rng.random(n) < p for p in (0.7, 0.6, 0.8))
    ld, rd, md = dev(lv), dev(rv), dev(mv)
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    pick = mv & mok
    want_ok = np.where(pick, lok, rok)
    want = np.where(pick, lv, rv)
    for lb, rb, mb in itertools.product(BEGIN_BITS, repeat=3):
        lm, rm, mm = shifted_mask(rng, lok, lb), shifted_mask(rng, rok, rb), shifted_mask(rng, mok, mb)
        out = torch.empty(n * 4, dtype=torch.uint8, device="cuda")
        out_valid = torch.full(((n + 511) // 512 * 16,), 0x33333333, dtype=torch.int32, device="cuda")
        nulls = torch.full((1,), -3, dtype=torch.int64, device="cuda")
        assert lib.gx_copy_if_else(4, ld.data_ptr(), lm.data_ptr(), lb, None, 0, rd.data_ptr(), rm.data_ptr(), rb, None, 0, md.data_ptr(),
                                   mm.data_ptr(), mb, n, out.data_ptr(), out_valid.data_ptr(), nulls.data_ptr(), s) == 0
        assert np.array_equal(out.cpu().numpy().view(np.int32), want), (lb, rb, mb)
        assert np.array_equal(unpack(out_valid, n), want_ok), (lb, rb, mb)
        assert not unpack(out_valid, (n + 31) // 32 * 32)[n:].any()
        assert int(nulls.item()) == int((~want_ok).sum()), (lb, rb, mb)


# ------------------------------------------------------------------------------------------------ DataFrame
def _frames(rng, lens):
    import pandas as pd
    out = []
    for n in lens:
        f = (rng.random(n) - 0.5) * 100
        f[rng.random(n) < 0.2] = np.nan                      # nulls on the device
        g = rng.integers(-1000, 1000, n).astype(np.float64)
        g[rng.random(n) < 0.3] = np.nan
        out.append(pd.DataFrame({"k": rng.integers(-5, 5, n).astype(np.int64), "f": f, "g": g,
                                 "h": rng.integers(0, 100, n).astype(np.int32)}))
    return out


def test_dataframe_concat_against_pandas(gx, T):
    import pandas as pd
    cudf_amd = gx[0]
    rng = np.random.default_rng(41)
    pdfs = _frames(rng, (T + 37, 65, 1, 2 * T - 1))
    got = cudf_amd.concat([cudf_amd.DataFrame.from_pandas(p) for p in pdfs])
    want = pd.concat(pdfs, ignore_index=True)
    assert got.columns == list(want.columns) and len(got) == len(want)
    assert got["f"].null_count == int(want["f"].isna().sum()) and got["k"].mask is None
    pd.testing.assert_frame_equal(got.to_pandas(), want, check_dtype=False, check_exact=True)
    one = cudf_amd.concat([cudf_amd.DataFrame.from_pandas(pdfs[1])])
    pd.testing.assert_frame_equal(one.to_pandas(), pdfs[1], check_dtype=False, check_exact=True)


@pytest.mark.parametrize("other_kind", ["scalar", "none", "frame"])
def test_dataframe_where_and_mask_against_pandas(gx, T, other_kind):
    import pandas as pd
    cudf_amd, Column, _ = gx
    rng = np.random.default_rng(42)
    n = T + 37
    pdf, opdf = _frames(rng, (n, n))
    cond = rng.random(n) < 0.5
    df, odf = cudf_amd.DataFrame.from_pandas(pdf), cudf_amd.DataFrame.from_pandas(opdf)
    other, pother = {"scalar": (7, 7), "none": (None, np.nan), "frame": (odf, opdf)}[other_kind]
    c = Column.from_numpy(cond)
    pcond = pd.DataFrame({name: cond for name in pdf.columns})
    pd.testing.assert_frame_equal(df.where(c, other).to_pandas(), pdf.where(pcond, pother), check_dtype=False, check_exact=True)
    pd.testing.assert_frame_equal(df.mask(c, other).to_pandas(), pdf.mask(pcond, pother), check_dtype=False, check_exact=True)
    # a null cond element counts as false
    cn = Column.from_numpy(np.ones(n, dtype=bool), cond)
    pd.testing.assert_frame_equal(df.where(cn, other).to_pandas(), pdf.where(pcond, pother), check_dtype=False, check_exact=True)


# ------------------------------------------------------------------------------------------------ the C++ surface
def test_cpp_surface_cases():
    """cudf::concatenate / concatenate_masks / scatter / copy_if_else on views made by cudf::slice and cudf::split, through libcudf.so"""
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "cudf_copying_tests")], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "21 run, 0 failed" in r.stdout
