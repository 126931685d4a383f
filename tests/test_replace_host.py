"""CPU: cudf::replace_nulls / replace_nans / clamp / find_and_replace_all / normalize_nans_and_zeros as far as they can be checked
without a device -- exported symbols, the argument checks of the gx_replace.hip entry points (fake pointers: nothing is launched),
the scratch query of the policy fill, the --host cases of the C++ surface, the argument checks of the Python surface, and a NumPy
model of the three-step protocol of gx_replace_nulls_policy (tile table -> two-level running max -> per-tile resolve with a
per-word table), checked against the one-line np.maximum.accumulate model exhaustively for both directions."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cudf_amd", "libcudf.so")
BIN = os.path.join(ROOT, "tests", "cpp", "cudf_replace_tests")

GX_EINVAL, GX_EDTYPE, GX_ETMP = -1, -2, -3
DTYPES = range(1, 12)
FLOATS = (9, 10)
NEW = ("gx_replace_tile_rows", "gx_find_and_replace_chunk", "gx_replace_nulls", "gx_replace_nulls_policy", "gx_replace_nans", "gx_clamp",
       "gx_find_and_replace", "gx_normalize_nans_and_zeros")
BAD_N = (-1, 2**31, 2**40)
A, B, C, D = (ctypes.c_void_p(x) for x in (0x10000, 0x20000, 0x30000, 0x40000))   # "device pointers" that are never dereferenced


def _build():
    import __graft_entry__ as ge
    ge.build()


@pytest.fixture(autouse=True, scope="module")
def _the_kernel_layer_has_the_family():
    _build()
    from cudf_amd import _lib
    assert hasattr(_lib.lib, "gx_replace_nulls_policy") and "gx_replace_nulls_policy" in _lib.EXPORTED


@pytest.fixture(scope="module")
def lib():
    from cudf_amd import _lib
    return _lib.lib


def test_libraries_export_the_replace_api():
    syms = subprocess.check_output(["nm", "-DC", "--defined-only", LIB], text=True)
    for s, overloads in (("cudf::replace_nulls(", 3), ("cudf::replace_nans(", 2), ("cudf::find_and_replace_all(", 1), ("cudf::clamp(", 2),
                         ("cudf::normalize_nans_and_zeros(", 2)):
        assert syms.count(s) == overloads, f"libcudf.so exports {syms.count(s)} overloads of {s}"
    und = subprocess.check_output(["nm", "-D", "--undefined-only", LIB], text=True)
    from cudf_amd import _lib
    for s in NEW[2:]:
        assert s in und
    for s in NEW:
        assert s in _lib.EXPORTED and hasattr(_lib.lib, s)


def test_tile_rows_and_chunk(lib):
    T = lib.gx_replace_tile_rows()
    assert T > 0 and T % 64 == 0          # a tile owns whole 64-row validity spans: one writer per word
    assert lib.gx_find_and_replace_chunk() > 0


def test_error_codes_mirror_the_header():
    text = open(os.path.join(ROOT, "include", "cudf_amd", "gx.h")).read()
    import re
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"GX_(EINVAL|EDTYPE|ETMP)\s*=\s*(-\d+)", text)}
    assert codes == {"EINVAL": GX_EINVAL, "EDTYPE": GX_EDTYPE, "ETMP": GX_ETMP}


def _rn(lib, fn="gx_replace_nulls", first=8, inp=A, ibit=0, repl=B, rbit=0, scalar=0, n=7, out=C, out_valid=None, in_valid=None):
    return getattr(lib, fn)(first, inp, in_valid, ibit, repl, None, rbit, None, scalar, n, out, out_valid, None, None)


def test_replace_nulls_and_nans_misuse_is_rejected_before_any_device_call(lib):
    for fn, first in (("gx_replace_nulls", 8), ("gx_replace_nans", 10)):
        for n in BAD_N:
            assert _rn(lib, fn, first, n=n) == GX_EINVAL, (fn, n)
        assert _rn(lib, fn, first, ibit=-1) == GX_EINVAL and _rn(lib, fn, first, rbit=-1) == GX_EINVAL
        assert _rn(lib, fn, first, inp=None) == GX_EINVAL and _rn(lib, fn, first, repl=None) == GX_EINVAL
        assert _rn(lib, fn, first, out=None) == GX_EINVAL
        for scalar in (0, 1):
            assert _rn(lib, fn, first, n=0, inp=None, repl=None, out=None, scalar=scalar) == 0
    for e in (0, 3, 5, 16, -1):
        assert _rn(lib, first=e) == GX_EDTYPE, e
    for d in list(range(1, 9)) + [11, 0, 12, 99, -3]:          # a non-float dtype, an unknown dtype
        assert _rn(lib, "gx_replace_nans", d) == GX_EDTYPE, d
    # a nullable input needs somewhere to write its nulls
    assert _rn(lib, "gx_replace_nans", 10, in_valid=D, out_valid=None) == GX_EINVAL


def _policy(lib, elem=8, inp=A, valid=B, bit=0, n=7, back=0, out=C, out_valid=D, tmp=ctypes.c_void_p(0x50000), nbytes=1 << 30):
    nb = ctypes.c_size_t(nbytes)
    return lib.gx_replace_nulls_policy(elem, inp, valid, bit, n, back, out, out_valid, None, tmp, ctypes.byref(nb), None), nb.value


def test_policy_fill_misuse_and_scratch_query(lib):
    for n in BAD_N:
        assert _policy(lib, n=n)[0] == GX_EINVAL and _policy(lib, n=n, tmp=None)[0] == GX_EINVAL
    assert _policy(lib, bit=-1)[0] == GX_EINVAL
    for e in (0, 3, 16):
        assert _policy(lib, elem=e)[0] == GX_EDTYPE
    for bad in ("inp", "valid", "out", "out_valid"):
        assert _policy(lib, **{bad: None})[0] == GX_EINVAL, bad
    assert lib.gx_replace_nulls_policy(8, A, B, 0, 7, 0, C, D, None, None, None, None) == GX_EINVAL    # no tmp_bytes
    for back in (0, 1):
        assert _policy(lib, n=0, inp=None, valid=None, out=None, out_valid=None, back=back)[0] == 0
    # the query: pure host arithmetic, monotone in n, the carry table only (4 bytes per tile and a top level)
    T = lib.gx_replace_tile_rows()
    sizes = []
    for n in (0, 1, T, T + 1, 10**6, 1025 * T, 10**8, 2**31 - 1):
        rc, nb = _policy(lib, n=n, tmp=None, nbytes=0)
        assert rc == 0, n
        sizes.append(nb)
    assert sizes == sorted(sizes) and sizes[-1] > 0
    assert sizes[-1] < 2 * 4 * (2**31 // T) + 4096                       # against 8 bytes per ROW of the scan-and-gather composition
    rc, need = _policy(lib, n=10**8, tmp=None, nbytes=0)
    assert _policy(lib, n=10**8, nbytes=need - 1)[0] == GX_ETMP
    assert _policy(lib, n=10**8, nbytes=0)[0] == GX_ETMP


def test_clamp_find_and_normalize_misuse_is_rejected_before_any_device_call(lib):
    def clamp(d=4, inp=A, n=7, out=C):
        return lib.gx_clamp(d, inp, n, B, None, None, B, None, None, out, None)

    def find(d=4, inp=A, ibit=0, n=7, old=B, new=B, nbit=0, m=3, out=C, in_valid=None, new_valid=None, out_valid=None):
        return lib.gx_find_and_replace(d, inp, in_valid, ibit, n, old, new, new_valid, nbit, m, out, out_valid, None, None)

    def norm(d=10, inp=A, n=7, out=C):
        return lib.gx_normalize_nans_and_zeros(d, inp, n, out, None)

    for n in BAD_N:
        assert clamp(n=n) == GX_EINVAL and find(n=n) == GX_EINVAL and norm(n=n) == GX_EINVAL and find(m=n) == GX_EINVAL
    for d in (0, 12, 99, -3):
        assert clamp(d=d) == GX_EDTYPE and find(d=d) == GX_EDTYPE and norm(d=d) == GX_EDTYPE
    for d in list(range(1, 9)) + [11]:
        assert norm(d=d) == GX_EDTYPE
    assert clamp(inp=None) == GX_EINVAL and clamp(out=None) == GX_EINVAL
    assert norm(inp=None) == GX_EINVAL and norm(out=None) == GX_EINVAL
    assert find(inp=None) == GX_EINVAL and find(out=None) == GX_EINVAL and find(old=None) == GX_EINVAL and find(new=None) == GX_EINVAL
    assert find(ibit=-1) == GX_EINVAL and find(nbit=-1) == GX_EINVAL
    assert find(in_valid=D) == GX_EINVAL and find(new_valid=D) == GX_EINVAL      # nulls possible, no out_valid
    for d in DTYPES:
        assert clamp(d=d, n=0, inp=None, out=None) == 0 and find(d=d, n=0, inp=None, out=None, old=None, new=None) == 0
    for d in FLOATS:
        assert norm(d=d, n=0, inp=None, out=None) == 0


def test_cpp_host_cases_run_without_a_device():
    """the throws of the C++ surface that do not need a device scalar, and the empty results: decided before the first device call"""
    _build()
    r = subprocess.run([BIN, "--host"], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "6 run, 0 failed" in r.stdout
    assert "[ OK ] size mismatches throw std::invalid_argument, and not cudf::data_type_error" in r.stdout
    assert "[ OK ] nulls in values_to_replace throw std::invalid_argument" in r.stdout


def test_python_surface_rejects_bad_arguments_without_a_device():
    """checks that come before the first allocation: a Column is only looked at"""
    import torch
    from cudf_amd import Column, DataFrame, ops

    def col(dtype, n=5, nulls=False):
        c = Column(torch.empty(0, dtype=torch.uint8), dtype, n)
        if nulls:
            c.mask, c.null_count = torch.empty(0, dtype=torch.int32), 1
        return c

    i32, i32n, f64, i64 = col("int32"), col("int32", nulls=True), col("float64"), col("int64")
    with pytest.raises(ValueError):
        ops.replace_nulls(i32n, "nearest")
    with pytest.raises(TypeError):
        ops.replace_nulls(i32n, i64)
    with pytest.raises(ValueError):
        ops.replace_nulls(i32n, col("int32", 4))
    for bad in (2**31, -2**31 - 1, 1.5):
        with pytest.raises(TypeError):
            ops.replace_nulls(i32n, bad)
        with pytest.raises(TypeError):
            ops.clamp(i32, bad, None)
        with pytest.raises(TypeError):
            ops.clamp(i32, None, 3, hi_replace=bad)
    with pytest.raises(TypeError):
        ops.replace_nulls(col("uint8", nulls=True), -1)
    with pytest.raises(TypeError):
        ops.replace_nans(i32, 0)
    with pytest.raises(TypeError):
        ops.normalize_nans_and_zeros(i32)
    with pytest.raises(TypeError):
        ops.find_and_replace_all(i32, i64, i32)
    with pytest.raises(ValueError):
        ops.find_and_replace_all(i32, i32, col("int32", 4))
    with pytest.raises(ValueError):
        ops.find_and_replace_all(i32, i32n, i32)
    with pytest.raises(ValueError):
        i32n.fillna()
    with pytest.raises(ValueError):
        i32n.fillna(1, method="ffill")
    with pytest.raises(ValueError):
        i32n.fillna(method="nearest")
    with pytest.raises(TypeError):
        i32n.fillna("x")
    with pytest.raises(ValueError):
        i32.replace([1, 2], [3])
    with pytest.raises(TypeError):
        i32.replace(1.5, 2)
    df = DataFrame()
    df._cols["a"] = i32n
    with pytest.raises(KeyError):
        df.fillna({"b": 1})
    with pytest.raises(TypeError):
        df.fillna(0.5)
    with pytest.raises(ValueError):
        df.fillna({"a": 1}, method="ffill")
    for name in ("fillna", "ffill", "bfill", "clip", "replace"):
        assert callable(getattr(Column, name)) and callable(getattr(DataFrame, name))


# ------------------------------------------------------------------------------------------------ the protocol of the policy fill
def one_line_model(valid, backward):
    """source row of every row (itself where it is valid), -1 where there is none"""
    n = len(valid)
    if not backward:
        return np.maximum.accumulate(np.where(valid, np.arange(n), -1)) if n else np.zeros(0, np.int64)
    rev = np.maximum.accumulate(np.where(valid[::-1], np.arange(n), -1)) if n else np.zeros(0, np.int64)
    return np.where(rev < 0, -1, n - 1 - rev)[::-1]


def bits_from(words, bit, cnt):
    """cnt bits of an LSB-first uint32 bitmap from `bit` on, as a bool array: what the kernel's readers return"""
    idx = bit + np.arange(cnt)
    return ((words[idx >> 5] >> (idx & 31).astype(np.uint32)) & 1).astype(bool)


def three_step_model(words, begin_bit, n, backward, tile, word, block):
    """gx_replace_nulls_policy as the kernels compute it: `tile` rows per tile, `word` rows per validity span of a tile (the per-word
    table), `block` table entries per workgroup of the carry pass.  Both directions through one key: PRECEDING key = row, entry =
    tile; FOLLOWING key = n - 1 - row, entry = tiles - 1 - tile; the nearest valid row behind a tile is the largest key below its entry."""
    assert tile % word == 0
    tiles = -(-n // tile)
    # 1. the tile table, from the bitmap alone
    table = np.full(tiles, -1, np.int64)
    for t in range(tiles):
        r0, r1 = t * tile, min((t + 1) * tile, n)
        hit = np.flatnonzero(bits_from(words, begin_bit + r0, r1 - r0))
        if len(hit):
            table[tiles - 1 - t if backward else t] = n - 1 - (r0 + hit[0]) if backward else r0 + hit[-1]
    # 2. exclusive running max: inside blocks of `block` entries, then over the blocks
    blocks = -(-tiles // block)
    local, top = np.full(tiles, -1, np.int64), np.full(blocks, -1, np.int64)
    for b in range(blocks):
        run = -1
        for e in range(b * block, min((b + 1) * block, tiles)):
            local[e] = run
            run = max(run, table[e])
        top[b] = run
    run = -1
    for b in range(blocks):
        top[b], run = run, max(run, top[b])
    # 3. every tile on its own
    src = np.full(n, -1, np.int64)
    nw = tile // word
    for t in range(tiles):
        t0 = t * tile
        e = tiles - 1 - t if backward else t
        ckey = max(local[e], top[e // block])
        carry = -1 if ckey < 0 else (n - 1 - ckey if backward else ckey)
        wbits, key = [], []
        for w in range(nw):
            r0 = t0 + w * word
            cnt = max(0, min(word, n - r0))
            b = np.zeros(word, bool)
            if cnt:
                b[:cnt] = bits_from(words, begin_bit + r0, cnt)
            hit = np.flatnonzero(b)
            wbits.append(b)
            key.append(-1 if not len(hit) else (tile - 1 - (w * word + hit[0]) if backward else w * word + hit[-1]))
        near = [-1] * nw                    # inclusive scan in fill direction
        run = -1
        for w in (range(nw - 1, -1, -1) if backward else range(nw)):
            run = max(run, key[w])
            near[w] = run
        for w in range(nw):
            for lane in range(word):
                r = t0 + w * word + lane
                if r >= n:
                    break
                b = wbits[w]
                if b[lane]:
                    src[r] = r
                    continue
                if backward:
                    above = np.flatnonzero(b[lane + 1:])
                    k = near[w + 1] if w + 1 < nw else -1
                    src[r] = r + 1 + above[0] if len(above) else (t0 + tile - 1 - k if k >= 0 else carry)
                else:
                    below = np.flatnonzero(b[:lane])
                    k = near[w - 1] if w > 0 else -1
                    src[r] = t0 + w * word + below[-1] if len(below) else (t0 + k if k >= 0 else carry)
    return src


def _words(valid, begin_bit, rng):
    """a bitmap that holds `valid` from begin_bit on, random bits around it"""
    total = begin_bit + len(valid)
    bits = rng.integers(0, 2, ((total + 31) // 32 + 1) * 32).astype(np.uint8)
    bits[begin_bit:total] = valid
    return np.packbits(bits, bitorder="little").view(np.uint32)


@pytest.mark.parametrize("backward", [False, True])
def test_three_step_protocol_all_bitmaps_up_to_12_rows(backward):
    rng = np.random.default_rng(1)
    for n in range(0, 13):
        for pattern in range(1 << n):
            valid = ((pattern >> np.arange(n)) & 1).astype(bool)
            begin = pattern % 3
            got = three_step_model(_words(valid, begin, rng), begin, n, backward, tile=4, word=2, block=2)
            assert np.array_equal(got, one_line_model(valid, backward)), (n, pattern)


@pytest.mark.parametrize("backward", [False, True])
def test_three_step_protocol_random_bitmaps_tile_64_begin_bits_0_to_33(backward):
    rng = np.random.default_rng(2)
    for begin in range(34):
        for n, p in ((1, 0.5), (63, 0.5), (64, 0.1), (65, 0.5), (64 * 5 + 17, 0.02), (64 * 9 + 1, 0.003), (64 * 4, 0.0), (64 * 3 + 5, 1.0)):
            valid = rng.random(n) < p
            got = three_step_model(_words(valid, begin, rng), begin, n, backward, tile=64, word=8, block=3)
            assert np.array_equal(got, one_line_model(valid, backward)), (begin, n, p)
