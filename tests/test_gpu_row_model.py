"""GPU: the element rules every multi-column key kernel shares (cudf_amd/csrc/gx_rows.hpp), pinned from outside.

1. ops.hash_rows64 against a NumPy restatement of its fold, bit for bit: the values are public (sharded callers rely on equal rows
   hashing equal across ranks), so a change of the hash is a change of behaviour.
2. One set of equality classes across operators: on a sorted float column full of -0.0 / +0.0 / infinities / denormals / NaNs of
   many payloads (and nulls over bytes that read as NaN), the class boundaries that gx_group_heads, unique, gx_dense_rank,
   rows_mismatch_count, lower_bound / upper_bound and distinct_count report all equal those of the oracle's row comparator."""
import numpy as np
import pytest

from oracle import cudf_oracle as orc

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
DTYPES = ["int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float32", "float64", "bool"]


@pytest.fixture(scope="module")
def gx():
    import cudf_amd
    from cudf_amd import Column, ops
    return cudf_amd, Column, ops


# ---------------------------------------------------------------------------------------------- special values
def _specials(dtype):
    """+-0, +-inf, denormals, NaNs of distinct payloads and both signs, a few ordinary numbers -- as bit patterns"""
    if np.dtype(dtype) == np.float64:
        u, sign, exp, q = np.uint64, 1 << 63, 0x7FF0000000000000, 0x7FF8000000000000
        nan_payloads = [q, q | 1, exp | 1, exp | 0x000FFFFFFFFFFFFF, q | 0xDEAD]
        denormals = [1, 0x000FFFFFFFFFFFFF, 0x0000000100000000]
    else:
        u, sign, exp, q = np.uint32, 1 << 31, 0x7F800000, 0x7FC00000
        nan_payloads = [q, q | 1, exp | 1, exp | 0x007FFFFF, q | 0xBEEF]
        denormals = [1, 0x007FFFFF, 0x00010000]
    bits = [0, sign, exp, exp | sign]
    bits += denormals + [d | sign for d in denormals]
    bits += nan_payloads + [p | sign for p in nan_payloads]
    ordinary = np.array([1.0, -1.0, 2.5, -2.5, 1e30, -1e30, 3.0], dtype=dtype).view(u)
    return np.concatenate([np.array(bits, dtype=u), ordinary]).view(dtype)


def _special_column(dtype, n, seed):
    """about n rows: every special value repeated an uneven number of times, shuffled"""
    rng = np.random.default_rng(seed)
    sp = _specials(dtype)
    reps = rng.integers(1, 2 * max(2, n // len(sp)), len(sp))
    v = np.repeat(sp, reps)
    return v[rng.permutation(len(v))]


# ---------------------------------------------------------------------------------------------- 1. hash_rows64
def _normalised_bits(col):
    """the element's bytes zero-extended to 64 bits; floats: +-0 -> 0, NaN -> the quiet NaN of the width"""
    c = np.ascontiguousarray(col)
    if c.dtype.kind == "f":
        u = np.dtype(f"u{c.dtype.itemsize}")
        b = c.view(u).copy()
        b[c == 0] = 0
        b[np.isnan(c)] = 0x7FF8000000000000 if c.dtype.itemsize == 8 else 0x7FC00000
        return b.astype(np.uint64)
    if c.dtype.kind == "b":
        return c.view(np.uint8).astype(np.uint64)
    return c.view(np.dtype(f"u{c.dtype.itemsize}")).astype(np.uint64)


def _hash_rows64_numpy(cols, seed):
    n = len(cols[0])
    h = np.full(n, seed & M64, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for c in cols:
            x = h + np.uint64(0x9E3779B97F4A7C15) + _normalised_bits(c)
            x ^= x >> np.uint64(33)
            x *= np.uint64(0xFF51AFD7ED558CCD)
            x ^= x >> np.uint64(33)
            x *= np.uint64(0xC4CEB9FE1A85EC53)
            x ^= x >> np.uint64(33)
            h = x ^ ((h << np.uint64(1)) | (h >> np.uint64(63)))
    return h


def _random_column(dtype, n, rng):
    dt = np.dtype(dtype)
    if dt.kind == "b":
        return rng.integers(0, 2, n).astype(bool)
    if dt.kind == "f":
        v = rng.standard_normal(n).astype(dt)
        sp = _specials(dt)
        k = min(n, len(sp))
        v[rng.permutation(n)[:k]] = sp[:k]  # the special values among ordinary ones
        return v
    return rng.integers(0, 1 << 64, n, dtype=np.uint64).astype(np.dtype(f"u{dt.itemsize}")).view(dt)


def _check_hash(gx, cols, seed):
    _, Column, ops = gx
    got = ops.hash_rows64([Column.from_numpy(c) for c in cols], seed=seed).to_numpy()
    np.testing.assert_array_equal(got, _hash_rows64_numpy(cols, seed))


@pytest.mark.parametrize("dtype", DTYPES)
def test_hash_rows64_single_column(gx, dtype):
    rng = np.random.default_rng(DTYPES.index(dtype))
    for n in (1, 255, 256, 257, 1025):
        _check_hash(gx, [_random_column(dtype, n, rng)], 0)


@pytest.mark.parametrize("seed", [0, 0xDEADBEEF])
@pytest.mark.parametrize("dtypes", [("int64", "int64"), ("int32", "uint16", "int8"), ("float32", "float64", "bool")], ids="-".join)
def test_hash_rows64_column_sets(gx, dtypes, seed):
    rng = np.random.default_rng(len(dtypes) + seed % 7)
    _check_hash(gx, [_random_column(d, 4099, rng) for d in dtypes], seed)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_hash_rows64_float_specials(gx, dtype):
    v = _special_column(dtype, 600, 3)
    _check_hash(gx, [v], 0)
    _check_hash(gx, [v, v[::-1].copy()], 0xDEADBEEF)
    # every zero hashes as +0 and every NaN as one NaN
    _, Column, ops = gx
    h = ops.hash_rows64([Column.from_numpy(v)]).to_numpy()
    assert len(set(h[v == 0].tolist())) == 1 and len(set(h[np.isnan(v)].tolist())) == 1


def test_hash_rows64_second_grid_trip(gx):
    """16384 workgroups x 256 threads x 4 rows is the capped grid's first trip: one row more than that, and a ragged tail"""
    n = 16384 * 256 * 4 + 257
    v = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)).view(np.int64)
    _check_hash(gx, [v], 0)


# ---------------------------------------------------------------------------------------------- 2. equality classes
def _oracle_heads(cols, valids):
    """heads[i] = row i of the SORTED table differs from row i - 1 under the oracle's row comparator (heads[0] = True)"""
    n = len(cols[0])
    heads = np.zeros(n, bool)
    heads[0] = True
    for c, v in zip(cols, valids):
        ok = np.ones(n, bool) if v is None else np.asarray(v, bool)
        bits = np.where(ok, orc.sortable_bits(c), 0)  # nulls are all equivalent, their bytes do not count
        heads[1:] |= (bits[1:] != bits[:-1]) | (ok[1:] != ok[:-1])
    return heads


def _class_bounds(heads):
    """per row: first row of its class, one past its last row"""
    n = len(heads)
    starts = np.flatnonzero(heads)
    ends = np.append(starts[1:], n)
    label = np.cumsum(heads) - 1
    return starts[label], ends[label]


def _i32(Column, a):
    return Column.from_numpy(np.asarray(a, dtype=np.int32))


def _check_unique(gx, cols, heads):
    _, Column, ops = gx
    n = len(heads)
    out = ops.unique(list(cols) + [_i32(Column, np.arange(n))], list(range(len(cols))), keep="first", nulls_equal=True)
    np.testing.assert_array_equal(out[-1].to_numpy(), np.flatnonzero(heads))


def _check_mismatch(gx, cols, heads):
    _, Column, ops = gx
    n = len(heads)
    rows = np.arange(1, n)
    assert ops.rows_mismatch_count(cols, cols, _i32(Column, rows), _i32(Column, rows - 1), n - 1) == int(heads[1:].sum())
    for want_differ in (True, False):  # the pairs at a boundary all differ, the pairs inside a class all agree
        r = rows[heads[1:] == want_differ]
        assert ops.rows_mismatch_count(cols, cols, _i32(Column, r), _i32(Column, r - 1), len(r)) == (len(r) if want_differ else 0)


def _check_bounds(gx, cols, heads):
    _, _, ops = gx
    first, past = _class_bounds(heads)
    lb, ub = ops.lower_bound(cols, cols).to_numpy(), ops.upper_bound(cols, cols).to_numpy()
    np.testing.assert_array_equal(lb, first)
    np.testing.assert_array_equal(ub, past)
    np.testing.assert_array_equal(np.flatnonzero(np.append(True, lb[1:] != lb[:-1])), np.flatnonzero(heads))


@pytest.mark.parametrize("dtype,with_nulls", [("float64", True), ("float32", False)], ids=["float64-nulls", "float32"])
def test_one_column_equality_classes(gx, dtype, with_nulls):
    cudf_amd, Column, ops = gx
    import torch
    v = _special_column(dtype, 600, 11)
    n = len(v)
    valid = None
    if with_nulls:  # nulls over bytes that would read as NaN, and over ordinary ones
        rng = np.random.default_rng(5)
        valid = np.ones(n, bool)
        nan_rows = np.flatnonzero(np.isnan(v))
        valid[nan_rows[::3]] = False
        valid[rng.permutation(n)[:17]] = False
    col = Column.from_numpy(v, valid)
    order = ops.sorted_order(col)
    scol = ops.gather(col, order)
    o = order.to_numpy()
    sv, svalid = v[o], (None if valid is None else valid[o])
    np.testing.assert_array_equal(scol.to_numpy().view(np.uint8), sv.view(np.uint8))
    heads = _oracle_heads([sv], [svalid])
    assert 10 < heads.sum() < n

    # (a) gx_group_heads
    got = torch.empty(n, dtype=torch.uint8, device="cuda")
    cudf_amd._lib.check(cudf_amd._lib.lib.gx_group_heads(scol.gx, scol.data_ptr, scol.mask_ptr, None, n, 0, ops.ptr(got),
                                                         ops.stream_ptr()), "gx_group_heads")
    np.testing.assert_array_equal(got.cpu().numpy().astype(bool), heads)
    # (b) unique
    _check_unique(gx, [scol], heads)
    # (c) gx_dense_rank: the id changes where the class does
    ids, _, ngroups = ops.dense_rank(scol)
    ids = ids.to_numpy()
    assert ngroups == int(heads.sum())
    np.testing.assert_array_equal(np.append(True, ids[1:] != ids[:-1]), heads)
    # (d) rows_mismatch_count (it does not look at bitmaps)
    if not with_nulls:
        _check_mismatch(gx, [scol], heads)
    # (e) lower_bound / upper_bound of the column in itself
    _check_bounds(gx, [scol], heads)
    assert ops.distinct_count([col]) == int(heads.sum())


def test_two_column_equality_classes(gx):
    _, Column, ops = gx
    f = _special_column("float64", 600, 23)
    n = len(f)
    k = np.random.default_rng(9).integers(-2, 2, n).astype(np.int32)
    cols = [Column.from_numpy(k), Column.from_numpy(f)]
    o = ops.sorted_order_table(cols).to_numpy()
    np.testing.assert_array_equal(o, orc.sorted_order_table([k, f]))
    sk, sf = k[o], f[o]
    scols = [Column.from_numpy(sk), Column.from_numpy(sf)]
    heads = _oracle_heads([sk, sf], [None, None])
    assert 40 < heads.sum() < n
    _check_unique(gx, scols, heads)
    _check_mismatch(gx, scols, heads)
    _check_bounds(gx, scols, heads)
    assert ops.distinct_count(cols) == int(heads.sum())
