"""CPU: cudf::interleave_columns / tile / transpose / fill / repeat / sequence as far as they can be checked without a device --
exported symbols, the argument checks of the gx_reshape.hip entry points (fake pointers: nothing is launched), the scratch queries,
the tile query of the interleave, the --host cases of the C++ surface, the argument checks of the Python surface, and two NumPy
models of what the kernels do: the validity-word composition of interleave / tile / repeat_each (the word loops of
k_interleave_valid and k_tile_repeat, with readers that fail on any word a call must not touch) against np.stack(...).ravel() /
np.tile / np.repeat, and the expansion protocol of gx_repeat_map (binary search, marks where the largest row wins, max-scan)
against np.repeat."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cudf_amd", "libcudf.so")
BIN = os.path.join(ROOT, "tests", "cpp", "cudf_reshape_tests")

GX_EINVAL, GX_EDTYPE, GX_ETMP = -1, -2, -3
NEW = ("gx_reshape_tile_rows", "gx_interleave_tile", "gx_interleave", "gx_tile", "gx_repeat_each", "gx_repeat_map", "gx_fill_range",
       "gx_sequence")
BAD_N = (-1, 2**31, 2**40)
A, B, C, D = (ctypes.c_void_p(x) for x in (0x10000, 0x20000, 0x30000, 0x40000))   # "device pointers" that are never dereferenced
LDS_BUDGET = 64 * 1024


def _build():
    import __graft_entry__ as ge
    ge.build()


@pytest.fixture(autouse=True, scope="module")
def _the_kernel_layer_has_the_family():
    _build()
    from cudf_amd import _lib
    assert hasattr(_lib.lib, "gx_interleave") and "gx_interleave" in _lib.EXPORTED


@pytest.fixture(scope="module")
def lib():
    from cudf_amd import _lib
    return _lib.lib


def test_libraries_export_the_reshape_api():
    syms = subprocess.check_output(["nm", "-DC", "--defined-only", LIB], text=True)
    for s, overloads in (("cudf::interleave_columns(", 1), ("cudf::tile(", 1), ("cudf::transpose(", 1), ("cudf::fill(", 1),
                         ("cudf::fill_in_place(", 1), ("cudf::repeat(", 2), ("cudf::sequence(", 2)):
        assert syms.count(s) == overloads, f"libcudf.so exports {syms.count(s)} overloads of {s}"
    und = subprocess.check_output(["nm", "-D", "--undefined-only", LIB], text=True)
    from cudf_amd import _lib
    for s in ("gx_interleave", "gx_tile", "gx_repeat_each", "gx_repeat_map", "gx_fill_range", "gx_sequence"):
        assert s in und
    for s in NEW:
        assert s in _lib.EXPORTED and hasattr(_lib.lib, s)
    for header in ("filling.hpp", "reshape.hpp", "transpose.hpp"):
        assert os.path.exists(os.path.join(ROOT, "include", "cudf", header))


def test_tile_rows(lib):
    T = lib.gx_reshape_tile_rows()
    assert T > 0 and T % 32 == 0          # a tile owns whole validity words: one writer per word


def _tile(lib, elem, ncols):
    r, c = ctypes.c_int(-1), ctypes.c_int(-1)
    return lib.gx_interleave_tile(elem, ncols, ctypes.byref(r), ctypes.byref(c)), r.value, c.value


def test_interleave_tile_fits_the_lds_budget(lib):
    for elem in (1, 2, 4, 8):
        for ncols in range(1, 4098):
            rc, r, c = _tile(lib, elem, ncols)
            assert rc == 0 and r > 0 and 0 < c <= ncols, (elem, ncols, rc, r, c)
            assert r * c * elem <= LDS_BUDGET, (elem, ncols, r, c)
            if c == ncols:
                assert r % 32 == 0, (elem, ncols, r)     # a band owns whole output words and starts 16-byte aligned
    assert _tile(lib, 4, 4097)[2] < 4097                   # a wide table is cut along its columns too
    for e in (0, 3, 16, -1):
        assert _tile(lib, e, 4)[0] == GX_EDTYPE
    for k in (0, -1):
        assert _tile(lib, 4, k)[0] == GX_EINVAL
    assert lib.gx_interleave_tile(4, 4, None, None) == GX_EINVAL


def _il(lib, elem=8, k=3, cols="ok", valid=None, bits=None, n=7, out=C, out_valid=None, tmp=D, nbytes=1 << 30):
    ptrs = (ctypes.c_void_p * max(k, 1))(*([0x10000] * max(k, 1))) if cols == "ok" else cols
    nb = ctypes.c_size_t(nbytes)
    return lib.gx_interleave(elem, k, ptrs, valid, bits, n, out, out_valid, None, tmp, ctypes.byref(nb), None), nb.value


def test_interleave_misuse_and_scratch_query(lib):
    for n in BAD_N:
        assert _il(lib, n=n)[0] == GX_EINVAL
    assert _il(lib, k=3, n=2**30)[0] == GX_EINVAL                 # 3 * 2^30 result rows
    assert _il(lib, k=2, n=2**30)[0] == GX_EINVAL                 # exactly 2^31
    for e in (0, 3, 16, -1):
        assert _il(lib, elem=e)[0] == GX_EDTYPE
    for k in (0, -1):
        assert _il(lib, k=k)[0] == GX_EINVAL
    assert _il(lib, cols=None)[0] == GX_EINVAL and _il(lib, out=None)[0] == GX_EINVAL
    assert _il(lib, cols=(ctypes.c_void_p * 3)(0x10000, None, 0x10000))[0] == GX_EINVAL
    assert _il(lib, bits=(ctypes.c_int64 * 3)(0, -1, 0))[0] == GX_EINVAL
    assert lib.gx_interleave(8, 3, None, None, None, 7, C, None, None, None, None, None) == GX_EINVAL    # no tmp_bytes
    assert _il(lib, n=0, out=None)[0] == 0
    sizes = []
    for k in (1, 2, 16, 17, 64, 65, 4096, 10**6):
        rc, nb = _il(lib, k=k, cols=None, tmp=None, nbytes=0)       # the query reads no array
        assert rc == 0 and nb >= 24 * k
        sizes.append(nb)
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    need = _il(lib, k=100, tmp=None, nbytes=0)[1]
    assert _il(lib, k=100, nbytes=need - 1)[0] == GX_ETMP and _il(lib, k=100, nbytes=0)[0] == GX_ETMP


def test_tile_and_repeat_each_misuse(lib):
    for name in ("gx_tile", "gx_repeat_each"):
        fn = getattr(lib, name)

        def call(elem=4, inp=A, valid=None, bit=0, n=7, count=3, out=C):
            return fn(elem, inp, valid, bit, n, count, out, None, None, None)

        for bad in BAD_N:
            assert call(n=bad) == GX_EINVAL and call(count=bad) == GX_EINVAL, (name, bad)
        assert call(n=2**16, count=2**15) == GX_EINVAL              # exactly 2^31 result rows
        assert call(bit=-1) == GX_EINVAL
        for e in (0, 3, 16, -1):
            assert call(elem=e) == GX_EDTYPE
        assert call(inp=None) == GX_EINVAL and call(out=None) == GX_EINVAL
        assert call(n=0, inp=None, out=None) == 0 and call(count=0, inp=None, out=None) == 0


def _map(lib, offsets=A, n=7, total=9, out=C, tmp=D, nbytes=1 << 20):
    nb = ctypes.c_size_t(nbytes)
    return lib.gx_repeat_map(offsets, n, total, out, tmp, ctypes.byref(nb), None), nb.value


def test_repeat_map_misuse_and_scratch_query(lib):
    for bad in BAD_N:
        assert _map(lib, n=bad)[0] == GX_EINVAL and _map(lib, total=bad)[0] == GX_EINVAL
    assert _map(lib, n=0, total=5)[0] == GX_EINVAL
    assert _map(lib, offsets=None)[0] == GX_EINVAL and _map(lib, out=None)[0] == GX_EINVAL
    assert lib.gx_repeat_map(A, 7, 9, C, None, None, None) == GX_EINVAL
    assert _map(lib, total=0, offsets=None, out=None)[0] == 0
    sizes = [_map(lib, n=n, total=t, tmp=None, nbytes=77) for n, t in ((1, 1), (10**3, 10**4), (10**6, 2**31 - 1))]
    assert all(rc == 0 for rc, _ in sizes)
    assert [nb for _, nb in sizes] == sorted(nb for _, nb in sizes)       # it needs none: the query never shrinks, and says so
    assert sizes[-1][1] == 0


def test_fill_range_and_sequence_misuse(lib):
    def fill(elem=4, data=A, b=1, e=5, value=B):
        return lib.gx_fill_range(elem, data, b, e, value, None)

    assert fill(b=-1) == GX_EINVAL and fill(b=6, e=5) == GX_EINVAL and fill(e=2**31) == GX_EINVAL
    for el in (0, 3, 16, -1):
        assert fill(elem=el) == GX_EDTYPE
    assert fill(data=None) == GX_EINVAL and fill(value=None) == GX_EINVAL
    assert fill(b=5, e=5, data=None, value=None) == 0

    def seq(d=4, out=A, n=7, init=B, step=C):
        return lib.gx_sequence(d, out, n, init, step, None)

    for bad in BAD_N:
        assert seq(n=bad) == GX_EINVAL
    for d in (11, 0, 12, 99, -3):                              # BOOL8, unknown
        assert seq(d=d) == GX_EDTYPE, d
    assert seq(out=None) == GX_EINVAL and seq(init=None) == GX_EINVAL
    for d in range(1, 11):
        assert seq(d=d, n=0, out=None, init=None, step=None) == 0


def test_header_declares_the_family_as_c99():
    """gx.h with the new section still compiles as C99 -pedantic -Werror"""
    src = '#include "cudf_amd/gx.h"\nint main(void) { return 0; }\n'
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_cpp_host_cases_run_without_a_device():
    """the throws of the C++ surface that need no device scalar, and the empty results: decided before the first device call"""
    _build()
    r = subprocess.run([BIN, "--host"], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "6 run, 0 failed" in r.stdout
    assert "[ OK ] a result beyond size_type throws std::overflow_error" in r.stdout
    assert "[ OK ] empty inputs give empty results of the input's types" in r.stdout


def test_python_surface_rejects_bad_arguments_without_a_device():
    """checks that come before the first allocation: a Column is only looked at"""
    import torch
    from cudf_amd import Column, DataFrame, ops

    def col(dtype, n=5, nulls=False):
        c = Column(torch.empty(0, dtype=torch.uint8), dtype, n)
        if nulls:
            c.mask, c.null_count = torch.empty(0, dtype=torch.int32), 1
        return c

    i32, i32n, f64, i64, u8 = col("int32"), col("int32", nulls=True), col("float64"), col("int64"), col("uint8")
    with pytest.raises(ValueError):
        ops.interleave_columns([])
    with pytest.raises(TypeError):
        ops.interleave_columns([i32, i64])
    with pytest.raises(ValueError):
        ops.interleave_columns([i32, col("int32", 4)])
    with pytest.raises(OverflowError):
        ops.interleave_columns([col("int8", 2**30), col("int8", 2**30)])
    with pytest.raises(TypeError):
        ops.transpose([i32, f64])
    for fn in (ops.tile, ops.repeat):
        with pytest.raises(ValueError):
            fn(i32, -1)
        with pytest.raises(OverflowError):
            fn(col("int8", 2**30), 2)
        with pytest.raises(TypeError):
            fn(i32, 1.5)
        with pytest.raises(ValueError):
            fn([i32, col("int32", 4)], 2)
    with pytest.raises(ValueError):
        ops.repeat(i32, f64)                      # not integral
    with pytest.raises(ValueError):
        ops.repeat(i32, col("bool"))
    with pytest.raises(ValueError):
        ops.repeat(i32, i32n)                     # nulls
    with pytest.raises(ValueError):
        ops.repeat(i32, col("int32", 4))          # length
    with pytest.raises(ValueError):
        ops.sequence(-1, 0)
    with pytest.raises(ValueError):
        ops.sequence(3, None, dtype="int32")
    with pytest.raises(OverflowError):
        ops.sequence(2**31, 0)
    for bad_dtype in ("bool", "datetime64[s]", "U3"):
        with pytest.raises(TypeError):
            ops.sequence(3, 0, 1, dtype=bad_dtype)
    with pytest.raises(TypeError):
        ops.sequence(3, 0, 1.5, dtype="int32")
    with pytest.raises(TypeError):
        ops.sequence(3, 300, 1, dtype="uint8")
    with pytest.raises(TypeError):
        ops.sequence(3.0, 0)
    for b, e in ((-1, 2), (0, 6), (3, 2)):
        with pytest.raises(IndexError):
            ops.fill(i32, b, e, 1)
    with pytest.raises(TypeError):
        ops.fill(i32, 0, 2, 1.5)
    with pytest.raises(TypeError):
        ops.fill(u8, 0, 2, -1)
    with pytest.raises(ValueError):
        Column.arange(0, 5, 0)
    with pytest.raises(TypeError):
        Column.arange(5, dtype="bool")
    with pytest.raises(ValueError):
        i32.repeat(-2)
    df = DataFrame()
    df._cols["a"], df._cols["b"] = i32, f64
    with pytest.raises(TypeError):
        df.T
    with pytest.raises(TypeError):
        df.transpose()
    with pytest.raises(TypeError):
        df.interleave_columns()
    with pytest.raises(ValueError):
        df.repeat(-1)
    with pytest.raises(ValueError):
        DataFrame().interleave_columns()
    for name in ("repeat", "interleave_columns", "transpose", "T"):
        assert hasattr(DataFrame, name)
    assert callable(Column.repeat) and callable(Column.arange)


# ------------------------------------------------------------------------------------------------ model: the validity words
def pack(valid, begin_bit, rng=None):
    """words that hold `valid` from begin_bit on and END at the last word a reader may touch; the bits around are random"""
    total = begin_bit + len(valid)
    bits = np.zeros(((total + 31) // 32) * 32, np.uint8) if rng is None else rng.integers(0, 2, ((total + 31) // 32) * 32).astype(np.uint8)
    bits[begin_bit:total] = valid
    return np.packbits(bits, bitorder="little").view(np.uint32)


def bits_from(words, bit, cnt):
    """gx_validity.hpp bits_from: cnt (1..32) bits from `bit` on; the second word only when the run crosses into it"""
    assert 1 <= cnt <= 32
    w, sh = bit >> 5, bit & 31
    two = int(words[w])
    if sh + cnt > 32:
        two |= int(words[w + 1]) << 32
    return (two >> sh) & ((1 << cnt) - 1)


def interleave_words(cols, nrows):
    """k_interleave_valid: cols = [(words or None, begin bit)]; one output word at a time"""
    ncols, total = len(cols), nrows * len(cols)
    out = []
    for w in range((total + 31) // 32):
        e0, e1, word = 32 * w, min(32 * w + 32, total), 0
        if ncols <= 32:
            i0, i1 = e0 // ncols, (e1 - 1) // ncols
            nr = i1 - i0 + 1
            for j, (m, bbit) in enumerate(cols):
                bits = bits_from(m, bbit + i0, nr) if m is not None else (1 << nr) - 1
                for ii in range(nr):
                    e = (i0 + ii) * ncols + j
                    if e0 <= e < e1:
                        word |= ((bits >> ii) & 1) << (e - e0)
        else:
            i, j = divmod(e0, ncols)
            for e in range(e0, e1):
                m, bbit = cols[j]
                if m is None or (int(m[(bbit + i) >> 5]) >> ((bbit + i) & 31)) & 1:
                    word |= 1 << (e - e0)
                j += 1
                if j == ncols:
                    i, j = i + 1, 0
        out.append(word)
    return np.array(out, np.uint32)


def tile_words(m, bbit, nrows, count):
    """k_tile_repeat<MODE 0>: runs of the input bitmap, wrapping at nrows"""
    total, out = nrows * count, []
    for w in range((total + 31) // 32):
        e0, e1, word = 32 * w, min(32 * w + 32, total), 0
        e, i = e0, e0 % nrows
        while e < e1:
            cnt = min(nrows - i, e1 - e)
            word |= bits_from(m, bbit + i, cnt) << (e - e0)
            e, i = e + cnt, 0
        out.append(word)
    return np.array(out, np.uint32)


def repeat_words(m, bbit, nrows, count):
    """k_tile_repeat<MODE 1>: the bits of the source rows under the word, each spread over the result rows of its row"""
    total, out = nrows * count, []
    for w in range((total + 31) // 32):
        e0, e1, word = 32 * w, min(32 * w + 32, total), 0
        i0 = e0 // count
        nr = (e1 - 1) // count - i0 + 1
        bits = bits_from(m, bbit + i0, nr)
        for ii in range(nr):
            a = (i0 + ii) * count
            lo, hi = max(a, e0), min(a + count, e1)
            if (bits >> ii) & 1:
                word |= ((1 << (hi - lo)) - 1) << (lo - e0)
        out.append(word)
    return np.array(out, np.uint32)


def want_words(valid):
    return pack(np.asarray(valid, bool), 0) if len(valid) else np.zeros(0, np.uint32)


def bitmaps_of(nbits):
    """every bitmap of nbits bits up to 12 bits; above, the bitmaps that pin a composition in which every output bit is a copy of
    one input bit: all zero, all one, every single bit and every single hole"""
    if nbits <= 12:
        for x in range(1 << nbits):
            yield np.array([(x >> b) & 1 for b in range(nbits)], bool)
        return
    yield np.zeros(nbits, bool)
    yield np.ones(nbits, bool)
    for b in range(nbits):
        one = np.zeros(nbits, bool)
        one[b] = True
        yield one
        yield ~one


def test_model_interleave_words_small_shapes():
    for ncols in (1, 2, 3):
        for nrows in range(1, 13):
            for flat in bitmaps_of(ncols * nrows):
                valids = flat.reshape(ncols, nrows)
                got = interleave_words([(pack(v, 0), 0) for v in valids], nrows)
                assert (got == want_words(np.stack(valids, axis=1).ravel())).all(), (ncols, nrows, flat)


def test_model_interleave_words_random_begin_bits_and_widths():
    rng = np.random.default_rng(0)
    for ncols in (1, 2, 3, 5, 8, 16, 17, 31, 32, 33, 40, 67):
        for nrows in (1, 2, 31, 33, 65):
            for trial in range(3):
                valids = [rng.integers(0, 2, nrows).astype(bool) if rng.integers(0, 4) else None for _ in range(ncols)]
                bbits = [int(rng.integers(0, 34)) for _ in range(ncols)]
                cols = [(None, 0) if v is None else (pack(v, b, rng), b) for v, b in zip(valids, bbits)]
                got = interleave_words(cols, nrows)
                want = np.stack([np.ones(nrows, bool) if v is None else v for v in valids], axis=1).ravel()
                assert (got == want_words(want)).all(), (ncols, nrows, bbits)


def test_model_tile_and_repeat_words():
    rng = np.random.default_rng(1)
    for nrows in range(1, 13):
        for valid in bitmaps_of(nrows):                                   # every bitmap
            for count in range(1, 7):
                assert (tile_words(pack(valid, 0), 0, nrows, count) == want_words(np.tile(valid, count))).all(), (nrows, count, valid)
                assert (repeat_words(pack(valid, 0), 0, nrows, count) == want_words(np.repeat(valid, count))).all(), (nrows, count, valid)
    for bbit in range(34):
        for nrows, count in ((1, 70), (3, 50), (31, 5), (32, 3), (33, 3), (100, 2), (7, 1), (70, 1), (5, 64), (5, 65)):
            valid = rng.integers(0, 2, nrows).astype(bool)
            m = pack(valid, bbit, rng)
            assert (tile_words(m, bbit, nrows, count) == want_words(np.tile(valid, count))).all(), (bbit, nrows, count)
            assert (repeat_words(m, bbit, nrows, count) == want_words(np.repeat(valid, count))).all(), (bbit, nrows, count)


# ------------------------------------------------------------------------------------------------ model: the expansion protocol
def repeat_find(offsets, nrows, e):
    """the LAST s in [0, nrows) with offsets[s] <= e"""
    lo, hi = 0, nrows
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if offsets[mid] <= e:
            lo = mid
        else:
            hi = mid
    return lo


def repeat_map_model(counts, tile):
    """k_repeat_map, one tile at a time and no tile looking at another: two binary searches, the marks, the running max"""
    n = len(counts)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    total = int(offsets[-1])
    out = np.full(total, -1, np.int64)
    for t0 in range(0, total, tile):
        t1 = min(t0 + tile, total)
        s0, s1 = repeat_find(offsets, n, t0), repeat_find(offsets, n, t1 - 1)
        marks = [0] * tile
        skipping = [0] * tile
        marks[0] = skipping[0] = s0
        for s in range(s0 + 1, s1 + 1):
            p = int(offsets[s])
            assert t0 < p < t1
            marks[p - t0] = max(marks[p - t0], s)                  # rows of count 0 share a position: the largest row wins
            if offsets[s + 1] != p:                               # the kernel's form: a row of count 0 loses to the row behind it
                assert skipping[p - t0] == 0 or p - t0 == 0
                skipping[p - t0] = s
        assert marks == skipping
        run = 0
        for e in range(t0, t1):
            run = max(run, marks[e - t0])
            out[e] = run
    return out


def test_model_repeat_map_every_small_count_vector():
    for n in range(0, 7):
        for counts in itertools.product(range(4), repeat=n):
            counts = np.array(counts, np.int64)
            got = repeat_map_model(counts, 8)
            want = np.repeat(np.arange(n), counts)
            assert (got == want).all(), counts


def test_model_repeat_map_skew():
    rng = np.random.default_rng(2)
    for counts in ([0, 0, 100, 0], [1] + [0] * 30 + [1], [0] * 9 + [17] + [0] * 9, [8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 16, 0, 3],
                   rng.integers(0, 8, 200), np.where(rng.integers(0, 10, 300) == 0, 40, 0)):
        counts = np.asarray(counts, np.int64)
        assert (repeat_map_model(counts, 8) == np.repeat(np.arange(len(counts)), counts)).all()
