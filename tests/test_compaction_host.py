"""CPU: the row-filter feature (apply_boolean_mask / drop_nulls / drop_nans) as far as it can be checked without a device --
exported symbols, scratch queries, argument checks of the C ABI and of the C++ surface, and a NumPy model of the bit arithmetic
the kernels of cudf_amd/csrc/gx_compact.hip rely on."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cudf_amd", "libcudf.so")
BIN = os.path.join(ROOT, "tests", "cpp", "cudf_compaction_tests")

GX_EINVAL, GX_EDTYPE = -1, -2


def _build():
    import __graft_entry__ as ge
    ge.build()


def test_host_library_exports_the_stream_compaction_api():
    _build()
    syms = subprocess.check_output(["nm", "-DC", "--defined-only", LIB], text=True)
    for s in ["cudf::apply_boolean_mask(", "cudf::drop_nulls(", "cudf::drop_nans("]:
        assert s in syms, f"libcudf.so does not export {s}"
    und = subprocess.check_output(["nm", "-D", "--undefined-only", LIB], text=True)
    for s in ["gx_select_mask", "gx_select_valid_count", "gx_select_not_nan", "gx_compact_column"]:
        assert s in und, f"libcudf.so has no reference to {s}"
    from cudf_amd import _lib
    for s in ["gx_select_mask", "gx_select_valid_count", "gx_select_not_nan", "gx_compact_column", "gx_compact_indices",
              "gx_compare_scalar", "gx_compact_plan_bytes"]:
        assert s in _lib.EXPORTED and hasattr(_lib.lib, s)


def _align256(x):
    return (x + 255) // 256 * 256


def _plan_bytes(n):
    """the plan: one selection bit per row in uint64 words (+ 1 spare word), one int64 start per 4096-row chunk (+ the total)"""
    return _align256(8 * ((n + 63) // 64 + 1)) + _align256(8 * ((n + 4095) // 4096 + 1))


def _queries():
    from cudf_amd import _lib as L
    lib = L.lib
    nb = ctypes.c_size_t(0)

    def q(name, *args):
        nb.value = 0
        rc = getattr(lib, name)(*args, None, None, ctypes.byref(nb), None)   # count_dev, sel_tmp, &bytes, stream
        return rc, nb.value

    return L, lib, q


def test_scratch_queries_without_a_device():
    L, lib, q = _queries()
    one = (ctypes.c_int * 1)(L.FLOAT64)
    queries = {
        "gx_select_mask": lambda n: q("gx_select_mask", None, None, 0, n),
        "gx_select_valid_count": lambda n: q("gx_select_valid_count", 2, None, None, n, 2),
        "gx_select_not_nan": lambda n: q("gx_select_not_nan", 1, one, None, None, None, n, 1, 0),
        "gx_compact_plan_bytes": lambda n: (0, lib.gx_compact_plan_bytes(n)),
    }
    for name, fn in queries.items():
        sizes = []
        for n in (0, 1000, 10**6, 10**9):
            rc, b = fn(n)
            assert rc == 0, (name, n, rc)
            assert b == _plan_bytes(n), (name, n, b)
            sizes.append(b)
        assert sizes == sorted(sizes) and sizes[0] > 0, (name, sizes)
        assert sizes[-1] < 0.2e9, (name, sizes)                 # n / 8 bytes of bits + n / 512 bytes of chunk starts at 1e9 rows
    assert _plan_bytes(10**9) == 125_000_192 + 1_953_280


def test_misuse_is_rejected_before_any_device_call():
    L, lib, q = _queries()
    f64 = (ctypes.c_int * 1)(L.FLOAT64)
    i32 = (ctypes.c_int * 1)(L.INT32)
    bad = (ctypes.c_int * 1)(99)
    for n in (-1, 2**31):
        assert q("gx_select_mask", None, None, 0, n)[0] == GX_EINVAL
        assert q("gx_select_valid_count", 1, None, None, n, 1)[0] == GX_EINVAL
        assert q("gx_select_not_nan", 1, f64, None, None, None, n, 1, 0)[0] == GX_EINVAL
        assert lib.gx_compact_column(8, None, None, 0, n, None, None, None, None, None) == GX_EINVAL
        assert lib.gx_compact_indices(n, None, None, None) == GX_EINVAL
        assert lib.gx_compare_scalar(L.INT32, None, None, n, L.CMP_EQ, 0, None, None) == GX_EINVAL
        assert lib.gx_compact_plan_bytes(n) == 0
    assert q("gx_select_mask", None, None, 0, 2**31 - 1)[0] == 0
    assert q("gx_select_mask", None, None, -3, 10)[0] == GX_EINVAL                       # negative begin bit
    assert q("gx_select_valid_count", 1, None, None, 10, -1)[0] == GX_EINVAL             # keep_threshold < 0
    assert q("gx_select_valid_count", 33, None, None, 10, 1)[0] == GX_EINVAL             # more than 32 key columns
    assert q("gx_select_not_nan", 1, f64, None, None, None, 10, -1, 0)[0] == GX_EINVAL
    assert q("gx_select_not_nan", 1, i32, None, None, None, 10, 1, 0)[0] == GX_EDTYPE    # NaN selector on an integer dtype
    assert q("gx_select_not_nan", 1, i32, None, None, None, 10, 1, 1)[0] == 0            # ... allowed where a null is what is missing
    assert q("gx_select_not_nan", 1, bad, None, None, None, 10, 1, 1)[0] == GX_EDTYPE
    for size in (0, 3, 5, 16):
        assert lib.gx_compact_column(size, None, None, 0, 10, None, None, None, None, None) == GX_EDTYPE
    assert lib.gx_compact_column(4, None, None, 0, 10, None, None, None, None, None) == GX_EINVAL     # null pointers with n > 0
    assert lib.gx_compact_column(4, None, None, 0, 0, None, None, None, None, None) == 0              # nothing to do
    assert lib.gx_compact_indices(10, None, None, None) == GX_EINVAL
    assert lib.gx_compact_indices(0, None, None, None) == 0
    assert lib.gx_compare_scalar(99, None, None, 10, L.CMP_EQ, 0, None, None) == GX_EDTYPE
    for cmp in (-1, 6, 100):
        assert lib.gx_compare_scalar(L.INT32, None, None, 10, cmp, 0, None, None) == GX_EINVAL        # unknown cmp
    assert lib.gx_compare_scalar(L.INT32, None, None, 0, L.CMP_GE, 0, None, None) == 0


def test_cpp_argument_checks_run_without_a_device():
    """wrong mask type, wrong mask length, key index out of range, non-float drop_nans key, negative threshold: thrown by the C++
    surface before its first device call (tests/cpp/cudf_compaction_tests --host)"""
    _build()
    r = subprocess.run([BIN, "--host"], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "0 failed" in r.stdout and "[ OK ] apply_boolean_mask argument checks" in r.stdout


# ------------------------------------------------------------------------------------------------ the bit arithmetic
CHUNK, WAVE = 4096, 64


def _ballot_words(sel):
    n = len(sel)
    bits = np.zeros((n + WAVE - 1) // WAVE * WAVE, dtype=np.uint8)
    bits[:n] = sel
    return np.packbits(bits, bitorder="little").view(np.uint64)


def _popcount(words):
    return np.unpackbits(words.view(np.uint8)).reshape(len(words), 64).sum(axis=1).astype(np.int64)


def _masks(rng, n):
    yield rng.random(n) < 0.5
    yield rng.random(n) < 1e-3
    yield rng.random(n) < 0.999
    yield np.zeros(n, dtype=bool)
    yield np.ones(n, dtype=bool)
    yield (np.arange(n) % 2).astype(bool)
    yield ((np.arange(n) // 10_000) % 2).astype(bool)


def test_output_position_is_chunk_start_plus_word_popcounts_plus_lower_lanes():
    """select -> scan -> scatter: the position of a selected row is (selected rows of earlier chunks) + (popcount of the earlier
    words of its chunk) + (popcount of the lower lanes of its word); writing row numbers there gives np.flatnonzero"""
    rng = np.random.default_rng(7)
    for n in (1, 63, 64, 65, 4095, 4096, 4097, 50_001):
        for sel in _masks(rng, n):
            words = _ballot_words(sel)
            pc = _popcount(words)
            nchunks = (n + CHUNK - 1) // CHUNK
            wpc = CHUNK // WAVE
            padded = np.zeros(nchunks * wpc, dtype=np.int64)
            padded[: len(pc)] = pc
            per_chunk = padded.reshape(nchunks, wpc)
            counts = per_chunk.sum(axis=1)
            starts = np.concatenate([[0], np.cumsum(counts)])                      # k_partials_scan: exclusive, total behind
            row_start = (np.cumsum(per_chunk, axis=1) - per_chunk).reshape(-1)      # the in-chunk exclusive popcount scan
            total = int(starts[-1])
            assert total == int(sel.sum())
            out = np.full(total, -1, dtype=np.int64)
            rows = np.flatnonzero(sel)
            w = rows // WAVE
            lane = rows % WAVE
            lower = np.array([bin(int(words[wi]) & ((1 << int(l)) - 1)).count("1") for wi, l in zip(w, lane)], dtype=np.int64)
            pos = starts[rows // CHUNK] + row_start[w] + lower
            out[pos] = rows
            assert np.array_equal(out, rows), n


def test_mask_bytes_sixteen_per_lane_make_the_same_ballot_words():
    """the BOOL8 selector reads 16 mask bytes per lane: the 16-bit non-zero masks of the four lanes of a quad, shifted by
    16 * (lane & 3) and ORed, are the ballot word of the quad's 64 rows"""
    rng = np.random.default_rng(3)
    mask = rng.integers(0, 4, 64 * 16 * 5, dtype=np.uint8) * rng.integers(0, 2, 64 * 16 * 5, dtype=np.uint8)
    want = _ballot_words(mask != 0)
    lanes = (mask.reshape(-1, 16) != 0)
    m16 = (lanes * (1 << np.arange(16))).sum(axis=1).astype(np.uint64)
    quads = m16.reshape(-1, 4)
    got = np.zeros(len(quads), dtype=np.uint64)
    for k in range(4):
        got |= quads[:, k] << np.uint64(16 * k)
    assert np.array_equal(got, want)


def test_compacted_validity_pieces_merge_into_32_bit_words_at_any_offset():
    """per 64-row word the kernel builds `piece` = the validity bits of the selected rows in rank order (popcount(word) bits) and ORs
    it into the zeroed output bitmap at bit P = output position of the word's first selected row: parts (piece << (P & 31)) low 32,
    next 32, and piece >> (64 - (P & 31)) go to words P >> 5, + 1, + 2.  The result is the packed valid[sel]; padding stays zero."""
    rng = np.random.default_rng(11)
    M64 = (1 << 64) - 1
    straddles = set()
    for n in (64, 200, 4097, 20_000):
        for sel in _masks(rng, n):
            valid = rng.random(n) < 0.7
            total = int(sel.sum())
            out = [0] * ((total + 31) // 32 + 3)
            pos = 0
            for w0 in range(0, n, WAVE):
                s, v = sel[w0:w0 + WAVE], valid[w0:w0 + WAVE]
                vv = v[s]                                                  # lane r receives the bit of the r-th selected lane
                cnt = len(vv)
                piece = sum(1 << j for j in range(cnt) if vv[j])
                sh = pos & 31
                lo = (piece << sh) & M64
                hi = (piece >> (64 - sh)) if sh else 0
                parts = [lo & 0xFFFFFFFF, lo >> 32, hi & 0xFFFFFFFF]
                assert hi < (1 << 32)
                straddles.add(sum(1 for p in parts if p))
                for k, p in enumerate(parts):
                    if p:
                        out[(pos >> 5) + k] |= p
                pos += cnt
            assert pos == total
            want = np.zeros(len(out) * 32, dtype=np.uint8)
            want[:total] = valid[sel]
            assert np.array_equal(np.array(out, dtype=np.uint32), np.packbits(want, bitorder="little").view(np.uint32))
    assert {1, 2, 3} <= straddles                                          # pieces inside one word, across two and across three
