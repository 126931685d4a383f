"""CPU: cudf::concatenate / scatter / copy_if_else / slice / split as far as they can be checked without a device -- exported
symbols, the argument checks of gx_concatenate / gx_scatter / gx_copy_if_else, the --host cases of the C++ surface, the argument
checks of the Python surface, and a NumPy model of how one tile of k_concat (cudf_amd/csrc/gx_copying.hip: concat_word; gx_validity.hpp: bits_from)
composes an output validity word from up to 32 inputs with arbitrary begin bits, checked exhaustively against np.concatenate of the
unpacked bits."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cudf_amd", "libcudf.so")
BIN = os.path.join(ROOT, "tests", "cpp", "cudf_copying_tests")

GX_EINVAL, GX_EDTYPE, GX_ETMP = -1, -2, -3


def _build():
    import __graft_entry__ as ge
    ge.build()


@pytest.fixture(autouse=True, scope="module")
def _the_kernel_layer_has_the_operators():
    """everything here, the model included, describes gx_concatenate and its siblings: without them there is nothing to pin"""
    _build()
    from cudf_amd import _lib
    assert hasattr(_lib.lib, "gx_concatenate") and "gx_concatenate" in _lib.EXPORTED


def test_libraries_export_the_copying_api():
    syms = subprocess.check_output(["nm", "-DC", "--defined-only", LIB], text=True)
    for s, overloads in (("cudf::concatenate(", 2), ("cudf::concatenate_masks(", 1), ("cudf::scatter(", 2), ("cudf::copy_if_else(", 4),
                         ("cudf::slice(", 4), ("cudf::split(", 4)):
        assert syms.count(s) == overloads, f"libcudf.so exports {syms.count(s)} overloads of {s}"
    und = subprocess.check_output(["nm", "-D", "--undefined-only", LIB], text=True)
    from cudf_amd import _lib
    for s in ("gx_concatenate", "gx_scatter", "gx_copy_if_else"):
        assert s in und
        assert s in _lib.EXPORTED and hasattr(_lib.lib, s)
    assert "gx_concat_tile_rows" in _lib.EXPORTED
    for h in ("copying.hpp", "concatenate.hpp"):
        assert os.path.exists(os.path.join(ROOT, "include", "cudf", h))


def test_tile_rows():
    from cudf_amd import _lib as L
    T = L.lib.gx_concat_tile_rows()
    assert T > 0 and T % 32 == 0          # a tile owns whole validity words: nothing is merged between workgroups


def _arrays(ptrs, rows, valid=None, bits=None):
    k = len(rows)
    return ((ctypes.c_void_p * k)(*ptrs), (ctypes.c_int64 * k)(*rows),
            (ctypes.c_void_p * k)(*valid) if valid is not None else None,
            (ctypes.c_int64 * k)(*bits) if bits is not None else None)


def test_concatenate_misuse_is_rejected_before_any_device_call():
    from cudf_amd import _lib as L
    lib = L.lib
    fake, out, tmp = 0x10000, ctypes.c_void_p(0x20000), ctypes.c_void_p(0x30000)
    nb = ctypes.c_size_t(0)

    def cat(es=8, k=2, ptrs=(fake, fake), rows=(3, 4), valid=None, bits=None, out=out, out_valid=None, tmp=tmp, nbytes=1 << 20, arrays=True):
        nb.value = nbytes
        a = _arrays(ptrs, rows, valid, bits) if arrays else (None, None, None, None)
        return lib.gx_concatenate(es, k, a[0], a[1], a[2], a[3], out, out_valid, None, tmp, ctypes.byref(nb), None)

    for es in (0, 3, 5, 16, -1):
        assert cat(es=es) == GX_EDTYPE, es
    assert cat(k=0) == GX_EINVAL and cat(k=-1) == GX_EINVAL
    assert lib.gx_concatenate(8, 2, None, None, None, None, out, None, None, tmp, None, None) == GX_EINVAL      # no tmp_bytes
    assert cat(arrays=False) == GX_EINVAL                                                                      # no host arrays
    assert cat(rows=(3, -1)) == GX_EINVAL
    assert cat(rows=(2**31 - 1, 1)) == GX_EINVAL and cat(rows=(2**30, 2**30)) == GX_EINVAL and cat(rows=(2**40, 0)) == GX_EINVAL
    assert cat(ptrs=(fake, None)) == GX_EINVAL                                                                 # rows without a buffer
    assert cat(bits=(0, -1), valid=(fake, fake)) == GX_EINVAL
    assert cat(out=None) == GX_EINVAL
    assert cat(nbytes=8) == GX_ETMP
    # the scratch query is host arithmetic and grows with the number of inputs
    sizes = []
    for k in (1, 17, 1025, 100000):
        nb.value = 0
        assert lib.gx_concatenate(1, k, None, None, None, None, None, None, None, None, ctypes.byref(nb), None) == 0
        sizes.append(nb.value)
    assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[-1] >= 100000 * 32
    # no rows: nothing is launched, whatever the pointers
    for es in (1, 2, 4, 8):
        assert cat(es=es, ptrs=(None, None), rows=(0, 0), out=None) == 0
    assert cat(k=1, ptrs=(None,), rows=(0,), out=None) == 0


def test_scatter_misuse_is_rejected_before_any_device_call():
    from cudf_amd import _lib as L
    lib = L.lib
    fake, fake2, fake3 = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000), ctypes.c_void_p(0x30000)

    def sc(es=4, src=fake, valid=None, bit=0, sv=None, scalar=0, smap=fake2, n=5, target=fake3, tvalid=None, rows=9):
        return lib.gx_scatter(es, src, valid, bit, sv, scalar, smap, n, target, tvalid, rows, None)

    for es in (0, 3, 16, -8):
        assert sc(es=es) == GX_EDTYPE, es
    for n in (-1, 2**31, 2**40):
        assert sc(n=n) == GX_EINVAL, n
        assert sc(rows=n) == GX_EINVAL, n
    assert sc(bit=-1) == GX_EINVAL
    assert sc(src=None) == GX_EINVAL and sc(smap=None) == GX_EINVAL and sc(target=None) == GX_EINVAL
    assert sc(rows=0) == GX_EINVAL                                  # rows to write, nowhere to write them
    for es in (1, 2, 4, 8):
        assert sc(es=es, n=0, src=None, smap=None, target=None, rows=0) == 0


def test_copy_if_else_misuse_is_rejected_before_any_device_call():
    from cudf_amd import _lib as L
    lib = L.lib
    a, b, m, o = (ctypes.c_void_p(x) for x in (0x10000, 0x20000, 0x30000, 0x40000))

    def cie(es=8, lhs=a, lbit=0, lscalar=0, rhs=b, rbit=0, rscalar=0, mask=m, mbit=0, n=7, out=o):
        return lib.gx_copy_if_else(es, lhs, None, lbit, None, lscalar, rhs, None, rbit, None, rscalar, mask, None, mbit, n, out, None, None, None)

    for es in (0, 3, 7, 16, -1):
        assert cie(es=es) == GX_EDTYPE, es
    for n in (-1, 2**31, 2**40):
        assert cie(n=n) == GX_EINVAL, n
    assert cie(lbit=-1) == GX_EINVAL and cie(rbit=-1) == GX_EINVAL and cie(mbit=-1) == GX_EINVAL
    assert cie(lhs=None) == GX_EINVAL and cie(rhs=None) == GX_EINVAL and cie(mask=None) == GX_EINVAL and cie(out=None) == GX_EINVAL
    for es in (1, 2, 4, 8):
        for ls, rs in itertools.product((0, 1), repeat=2):
            assert cie(es=es, n=0, lhs=None, rhs=None, mask=None, out=None, lscalar=ls, rscalar=rs) == 0


def test_cpp_host_cases_run_without_a_device():
    """every throw of the C++ surface, the size_type overflow on views of fake pointers, slice index validation and the empty results:
    decided before the first device call (tests/cpp/cudf_copying_tests --host)"""
    _build()
    r = subprocess.run([BIN, "--host"], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "9 run, 0 failed" in r.stdout
    assert "[ OK ] concatenate: more rows than size_type holds throw std::overflow_error before any device call" in r.stdout
    assert "[ OK ] slice / split: an odd number of indices, begin > end and indices out of range throw" in r.stdout


def test_python_surface_rejects_bad_arguments_without_a_device():
    import cudf_amd
    from cudf_amd import Column, DataFrame, ops
    i64, i32, f64, b = (lambda n, dt=dt: Column(None, dt, n) for dt in (np.int64, np.int32, np.float64, np.bool_))
    with pytest.raises(ValueError):
        ops.concatenate([])
    with pytest.raises(TypeError):
        ops.concatenate([i64(3), i32(3)])
    with pytest.raises(OverflowError):
        ops.concatenate([Column(None, np.int8, 2**30), Column(None, np.int8, 2**30)])
    with pytest.raises(TypeError):
        ops.concatenate([Column(None, np.complex64, 3)])
    with pytest.raises(ValueError):
        ops.concatenate_tables([])
    with pytest.raises(ValueError):
        ops.concatenate_tables([[i64(3), i32(3)], [i64(2)]])
    with pytest.raises(TypeError):
        ops.concatenate_tables([[i64(3), i32(3)], [i64(2), f64(2)]])
    # scatter
    with pytest.raises(ValueError):
        ops.scatter([i64(3), i64(3)], i32(2), [i64(5)])
    with pytest.raises(TypeError):
        ops.scatter([i64(3)], i64(2), [i64(5)])                        # the map must be INT32
    with pytest.raises(ValueError):
        ops.scatter([i64(3)], Column(None, np.int32, 2, mask=object()), [i64(5)])   # ... without a mask
    with pytest.raises(TypeError):
        ops.scatter([i64(3)], i32(2), [f64(5)])
    with pytest.raises(ValueError):
        ops.scatter([i64(3)], i32(4), [i64(5)])                        # a map longer than the source
    with pytest.raises(ValueError):
        ops.scatter_scalar([1, 2], None, i32(2), [i64(5)])
    with pytest.raises(TypeError):
        ops.scatter_scalar([1], None, f64(2), [i64(5)])
    # copy_if_else
    with pytest.raises(TypeError):
        ops.copy_if_else(i64(4), i64(4), i64(4))                       # the mask must be BOOL8
    with pytest.raises(TypeError):
        ops.copy_if_else(i64(4), f64(4), b(4))
    with pytest.raises(ValueError):
        ops.copy_if_else(i64(4), i64(3), b(4))
    with pytest.raises(ValueError):
        ops.copy_if_else(i64(4), 1, b(5))
    with pytest.raises(TypeError):
        ops.copy_if_else(None, None, b(4))
    # the frame
    with pytest.raises(ValueError):
        cudf_amd.concat([])

    def frame(**cols):
        df = DataFrame()
        df._cols.update(cols)
        return df

    with pytest.raises(ValueError):
        cudf_amd.concat([frame(a=i64(2), b=f64(2)), frame(a=i64(3))])
    with pytest.raises(ValueError):
        cudf_amd.concat([frame(a=i64(2), b=f64(2)), frame(b=f64(3), a=i64(3))])
    with pytest.raises(TypeError):
        cudf_amd.concat([frame(a=i64(2)), frame(a=i32(3))])
    with pytest.raises(TypeError):
        cudf_amd.concat([frame(a=i64(2)), {"a": 1}])
    df = frame(a=i64(4), b=f64(4))
    with pytest.raises(TypeError):
        df.where(i64(4), 0)
    with pytest.raises(ValueError):
        df.where(b(5), 0)
    with pytest.raises(ValueError):
        df.mask(b(4), frame(a=i64(4)))
    with pytest.raises(TypeError):
        df.mask(b(4), frame(a=i64(4), b=i64(4)))
    with pytest.raises(TypeError):
        df.where(b(4), [1, 2, 3, 4])


# ------------------------------------------------------------------------------------------------ the model of one validity word
# inputs: (words, begin_bit, rows) with words = None for an input without nulls.  The model mirrors the device code line by line:
# concat_find (the LAST input that starts at or before the row), the walk over start[k + 1], bits_from of gx_validity.hpp (two words only
# when the run crosses a word), the shift into place.

def _find(start, lo, hi, r):
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if start[mid] <= r:
            lo = mid
        else:
            hi = mid
    return lo


def _bits_from(words, sb, cnt, reads):
    w, sh = sb >> 5, sb & 31
    reads.append(w)
    two = int(words[w])
    if sh + cnt > 32:
        reads.append(w + 1)
        two |= int(words[w + 1]) << 32
    v = (two >> sh) & 0xFFFFFFFF
    return v if cnt == 32 else v & ((1 << cnt) - 1)


def _model_word(inputs, start, r0, r1):
    k = _find(start, 0, len(inputs), r0)
    word, r = 0, r0
    while r < r1:
        e = min(start[k + 1], r1)
        if e > r:
            cnt = e - r
            words, bbit, _ = inputs[k]
            if words is None:
                bits = (1 << cnt) - 1
            else:
                reads = []
                bits = _bits_from(words, bbit + (r - start[k]), cnt, reads)
                assert max(reads) <= (bbit + inputs[k][2] - 1) >> 5      # no word behind the input's last bit is read
            word |= bits << (r - r0)
            r = e
        k += 1
    return word


def _pack(bits):
    pad = np.zeros((len(bits) + 31) // 32 * 32, dtype=np.uint8)
    pad[:len(bits)] = bits
    return np.packbits(pad, bitorder="little").view(np.uint32)


def _make_input(rng, rows, begin_bit, nullable):
    """(words, begin_bit, rows), the unpacked validity of its rows; the buffer holds noise in front of and behind the rows"""
    if not nullable:
        return (None, begin_bit, rows), np.ones(rows, dtype=np.uint8)
    buf = rng.integers(0, 2, begin_bit + rows + rng.integers(0, 3)).astype(np.uint8)
    if begin_bit + rows == 0:
        buf = np.zeros(0, dtype=np.uint8)
    return (_pack(buf), begin_bit, rows), buf[begin_bit:begin_bit + rows].copy()


def _check_concat(inputs, truth):
    rows = [i[2] for i in inputs]
    start = np.concatenate([[0], np.cumsum(rows)]).tolist()
    n = start[-1]
    want = np.concatenate(truth) if truth else np.zeros(0, dtype=np.uint8)
    assert len(want) == n
    got = [_model_word(inputs, start, r0, min(r0 + 32, n)) for r0 in range(0, n, 32)]
    want_words = _pack(want)
    assert [int(w) for w in want_words[:len(got)]] == got, (rows, [i[1] for i in inputs])


def test_model_of_a_validity_word_every_length_and_begin_bit():
    """two and three inputs of 0 ... 5 rows at every begin bit 0 ... 33, at the start of a word and behind a run of 31 rows,
    where they cross the word boundary"""
    rng = np.random.default_rng(3)
    cases = 0
    for lead in (0, 31):
        head, head_bits = _make_input(rng, lead, 5, lead % 2 == 1)
        for la, lb in itertools.product(range(6), repeat=2):
            for ba, bb in itertools.product(range(34), repeat=2):
                a, ta = _make_input(rng, la, ba, True)
                b, tb = _make_input(rng, lb, bb, True)
                _check_concat([head, a, b], [head_bits, ta, tb])
                cases += 1
    assert cases == 2 * 36 * 34 * 34


def test_model_of_a_validity_word_fed_by_32_inputs():
    """words assembled from up to 32 inputs of one row each, inputs without rows in between (also in front and at the end), inputs
    without a mask among them, begin bits 0 ... 33"""
    rng = np.random.default_rng(4)
    for trial in range(400):
        inputs, truth = [], []
        for _ in range(rng.integers(1, 90)):
            rows = int(rng.choice((0, 0, 1, 1, 1, 2, 3, 4, 5)))
            i, t = _make_input(rng, rows, int(rng.integers(0, 34)), rng.random() < 0.8)
            inputs.append(i)
            truth.append(t)
        _check_concat(inputs, truth)
    # exactly 32 inputs of one row in one word, 31 empty inputs between each pair
    inputs, truth = [], []
    for j in range(64):
        for rows in [1] + [0] * 31:
            i, t = _make_input(rng, rows, (7 * j) % 34, True)
            inputs.append(i)
            truth.append(t)
    _check_concat(inputs, truth)


def test_model_long_inputs_cross_many_words():
    rng = np.random.default_rng(5)
    for la, lb, lc in ((31, 33, 64), (32, 32, 32), (63, 1, 65), (100, 0, 29), (0, 0, 97), (1, 200, 0)):
        for bits in itertools.product((0, 1, 31, 33), repeat=3):
            made = [_make_input(rng, r, bb, True) for r, bb in zip((la, lb, lc), bits)]
            _check_concat([m[0] for m in made], [m[1] for m in made])
