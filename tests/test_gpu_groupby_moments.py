"""Groupby VARIANCE / STD / M2 against the exact moments, on every path that computes them.

The inputs (tests/moments_cases.py) are dyadic values whose exact moments come from Python integers: constant groups, large means
with small spreads, mean zero over 40 binades, the float32 analogues, groups holding a NaN or infinities, group sizes on both sides
of the wave / tile / scan-chunk sizes and one group of 50 021 rows, with and without null keys and null values, ddof 0 / 1 / 2.
The contract asserted for float values (u = 2^-53): |M2 - M2*| <= 16u M2* + 64u^2 S2*, M2 >= 0, VAR and STD within 4 further ulps,
never negative / NaN for finite values, NaN (valid) for a group holding a NaN or an infinity; for integer values with
sum x^2 < 2^53: |M2 - M2*| <= 8u S2* and M2 >= 0.  tests/test_groupby_moments_host.py shows that this check rejects the one-pass
formula sum x^2 - (sum x)^2 / c on the constant and the large-mean families and passes a plain two-pass below half the tolerance.

Paths: ops.groupby_var_std under both pinned hash algorithms and on the direct-address path of dense ids (read back from the
plan), cudf::groupby::aggregate on its hash path and on its sort path three ways (a request that forces it, pre-sorted keys,
null keys kept: the null-key group comes last and is checked too), DataFrame.groupby().var() / .std(); and the finalising kernel
gx_var_from_sums and the centring kernel gx_square_centered through the C ABI, bit for bit against NumPy.

With M2 = sum x^2 - (sum x)^2 / c for float values (the code before the centred second pass) all 25 cases of the first four tests
fail on an MI355X, each at its first assertion on the values: a negative M2 in 25 (31 with nulls) of the 199 finite float64 groups
and in 8 (11) of the 45 float32 groups -- constant groups and groups with a large mean.  With the centred pass the worst
|M2 - M2*| is 0.11 of the tolerance on every path (printed per case).

GPU time (MI355X): the 65 cases take 4 s together, 1.6 s of it the first import; the dense-id case (4.4e6 rows) 0.2 s, the
finalising kernel at 1 048 641 groups 0.15 s, every other case below 0.1 s.  The exact references are computed once per dtype and
mask and shared (0.3 s on the host for the float64 column).
"""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import cudf_oracle as orc
from tests import moments_cases as mc
from tests import route_values as route
from tests.test_gpu_cpp_parity import Dev, Out, NPT, shim  # noqa: F401  (the shim fixture and the device-column helpers)
from tests.test_gpu_join_groupby import _groupby_raw

M2, VARIANCE, STD = 11, 12, 13  # cudf::aggregation::Kind
FLOATS = ["float64", "float32"]


@pytest.fixture(scope="module")
def gx():
    import torch
    assert torch.cuda.is_available()
    import cudf_amd  # noqa: F401
    from cudf_amd import Column, ops
    return Column, ops


@pytest.fixture(params=[1, 2], ids=["global_table", "lds_partitioned"])
def gb_algo(request):
    """1 = global-atomic table, 2 = hash partitions + LDS tables for every n > 0"""
    from cudf_amd import _lib
    _lib.lib.gx_groupby_set_algorithm(request.param, 1)
    yield request.param
    _lib.lib.gx_groupby_set_algorithm(0, 1)


@functools.lru_cache(maxsize=None)
def _data(dtype):
    return mc.Moments(dtype)


def _valid(col):
    return col.valid_numpy() if col.mask is not None else np.ones(col.size, bool)


def _check_var_std(ds, ref, K, V, ops, ddof, want_keys, what):
    k, var, std, m2, cv = ops.groupby_var_std(K, V, ddof=ddof)
    np.testing.assert_array_equal(k.to_numpy(), want_keys)
    np.testing.assert_array_equal(cv.to_numpy(), ref["count"])
    for kind, col in (("m2", m2), ("var", var), ("std", std)):
        assert col.dtype == np.float64
        valid = _valid(col)
        assert col.null_count == int((~valid).sum())
        worst = mc.check(ref, kind, col.to_numpy(), valid, ddof, f"{what} ddof={ddof}")
        if kind == "m2":
            print(f"{what} ddof={ddof}: worst |M2 - M2*| / tolerance = {worst:.3g}")


@pytest.mark.parametrize("nulls", [False, True], ids=["nonulls", "nulls"])
@pytest.mark.parametrize("dtype", FLOATS)
def test_ops_groupby_var_std_pinned_hash_paths(gx, gb_algo, dtype, nulls):
    Column, ops = gx
    ds = _data(dtype)
    ref = ds.reference(nulls)
    keys = ds.keys(np.int64, 3, -100)
    K = Column.from_numpy(keys, ds.keys_valid if nulls else None)
    V = Column.from_numpy(ds.values(nulls), ds.values_valid if nulls else None)
    want_keys = ds.key_of_group[ref["group"]] * 3 - 100
    for ddof in (0, 1, 2):
        _check_var_std(ds, ref, K, V, ops, ddof, want_keys, f"{dtype} algorithm {gb_algo}")


def test_ops_groupby_var_std_dense_ids_by_direct_address(gx):
    """both SUM passes of the float path on the direct-address path of dense int32 ids (from 2^22 rows, no nulls): the column 15
    times, every copy under ids of its own"""
    Column, ops = gx
    from cudf_amd import _lib as L
    ds = _data("float64")
    ref = ds.reference(False)
    reps = 15
    assert reps * ds.n >= 1 << 22
    rng = np.random.default_rng(5)
    order = rng.permutation(reps * ds.n)
    keys = np.concatenate([ds.keys(np.int32, 1, r * ds.ngroups) for r in range(reps)])[order]
    vals = np.tile(ds.x, reps)[order]
    info = _groupby_raw(Column, ops, L, keys, vals)[4]
    assert info[0] == 1 and info[1] == 0, f"the dense path was not taken / fell back ({info})"
    k, var, std, m2, cv = ops.groupby_var_std(Column.from_numpy(keys), Column.from_numpy(vals))
    np.testing.assert_array_equal(k.to_numpy(), np.arange(reps * ds.ngroups))
    for kind, col in (("m2", m2), ("var", var), ("std", std)):
        got, valid = col.to_numpy().reshape(reps, -1), _valid(col).reshape(reps, -1)
        for r in range(reps):
            mc.check(ref, kind, got[r], valid[r], 1, f"dense ids, copy {r}")


def _cpp_aggregate(shim_call, keys, kvalid, vals, vvalid, kind, ddof, null_include, keys_sorted, force_sort):
    n = len(keys)
    dk, dv = Dev(keys, kvalid), Dev(vals, vvalid)
    ok_, ov = Out(np.int32, n, True), Out(np.float64, n, True)
    kn, vn, g, vt = ctypes.c_int(), ctypes.c_int(-1), ctypes.c_int(), ctypes.c_int()
    shim_call("shim_groupby_aggregate", dk.tid, dk.p, dk.mp, dk.nulls, dv.tid, dv.p, dv.mp, dv.nulls, n, kind, ddof, null_include, keys_sorted,
              force_sort, ok_.p, ok_.mp, ctypes.byref(kn), ov.p, ov.mp, ctypes.byref(vn), ctypes.byref(g), ctypes.byref(vt))
    G = g.value
    assert NPT[vt.value] == np.float64
    valid = ov.valid(G)
    assert vn.value == int((~valid).sum())
    return ok_.get(G), ok_.valid(G), ov.get(G), valid


CPP_PATHS = [("hash", False), ("hash", True), ("force_sort", False), ("force_sort", True), ("keys_sorted", False), ("keys_sorted", True),
             ("null_include", True)]


@pytest.mark.parametrize("path,nulls", CPP_PATHS, ids=[f"{p}-{'nulls' if n else 'nonulls'}" for p, n in CPP_PATHS])
@pytest.mark.parametrize("dtype", FLOATS)
def test_cpp_groupby_aggregate_hash_and_sort_paths(shim, dtype, path, nulls):  # noqa: F811
    ds = _data(dtype)
    null_group = path == "null_include"
    ref = ds.reference(nulls, null_group)
    keys, vals = ds.keys(np.int32, 3, -100), ds.values(nulls)
    kvalid, vvalid = (ds.keys_valid, ds.values_valid) if nulls else (None, None)
    if path == "keys_sorted":  # sorted::YES: keys already in order (the rows with a null key dropped: they would be sorted otherwise)
        if nulls:
            keys, vals, vvalid, kvalid = keys[kvalid], vals[kvalid], vvalid[kvalid], None
        o = np.argsort(keys, kind="stable")
        keys, vals, vvalid = keys[o], vals[o], None if vvalid is None else vvalid[o]
    want_keys = ds.key_of_group[ref["group"]] * 3 - 100
    want_kvalid = ref["group"] >= 0                        # the null-key group comes last
    flags = dict(null_include=int(null_group), keys_sorted=int(path == "keys_sorted"), force_sort=int(path == "force_sort"))
    for kind, name, ddofs in ((M2, "m2", (0,)), (VARIANCE, "var", (0, 1, 2)), (STD, "std", (0, 1, 2))):
        for ddof in ddofs:
            k, kv, got, valid = _cpp_aggregate(shim, keys, kvalid, vals, vvalid, kind, ddof, **flags)
            np.testing.assert_array_equal(kv, want_kvalid)
            np.testing.assert_array_equal(k[kv], want_keys[want_kvalid])
            worst = mc.check(ref, name, got, valid, ddof, f"{dtype} {path} {name} ddof={ddof}")
            if kind == M2:
                print(f"{dtype} {path} nulls={nulls}: worst |M2 - M2*| / tolerance = {worst:.3g}")


@pytest.mark.parametrize("families", [("const_",), ("centre_1e+08",)], ids=["constant", "large_mean"])
def test_dataframe_groupby_var_std(gx, families):
    from cudf_amd import DataFrame
    ds = mc.Moments("float64", families=families)
    ref = ds.reference(False)
    g = DataFrame({"k": ds.keys(np.int32), "v": ds.x}).groupby("k")
    for kind, out in (("var", g.var()), ("std", g.std())):
        np.testing.assert_array_equal(out["k"].to_numpy(), ds.key_of_group[ref["group"]])
        mc.check(ref, kind, out["v"].to_numpy(), _valid(out["v"]), 1, f"DataFrame {kind}")


# ---------------------------------------------------------------------------------------------------------------------
# integer values: the reference's arithmetic (int64 sums, the formula in double), pinned while sum x^2 < 2^53
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _integers(vdtype):
    rng = np.random.default_rng(77)
    info = np.iinfo(vdtype)
    centre, spread = {"int8": (0, 127), "int32": (30_000, 5), "int64": (-(1 << 20), 1000)}[vdtype]
    gens = [lambda c: rng.integers(centre - spread, centre + spread + 1, c), lambda c: np.full(c, int(info.max) if vdtype == "int8" else centre),
            lambda c: np.full(c, int(info.min) if vdtype == "int8" else -centre + 1)]
    vals, gid = [], []
    for gen in gens:
        for c in mc.COUNTS:
            gid.append(np.full(c, len(gid)))
            vals.append(gen(c))
    vals, gid = np.concatenate(vals).astype(vdtype), np.concatenate(gid)
    o = rng.permutation(len(vals))
    vals, gid = vals[o], gid[o]
    vv = rng.random(len(vals)) >= 0.15
    m2, s2, c = orc.exact_m2(vals, 0, np.where(vv, gid, -1), int(gid.max()) + 1)
    assert s2.max() < 2.0**53
    s1 = np.zeros(len(c), np.int64)
    np.add.at(s1, gid[vv], vals[vv].astype(np.int64))
    exact_square = np.array([int(s) ** 2 < 2**53 for s in s1])
    assert exact_square.sum() >= len(c) // 2
    return vals, gid.astype(np.int32), vv, m2, s2, c, exact_square


def _check_integer_m2(got, m2, s2, exact_square, what):
    assert np.all(np.abs(got - m2) <= 8 * mc.U * s2), f"{what}: M2 outside 8u S2*"
    assert (got[exact_square] >= 0).all(), f"{what}: negative M2"


@pytest.mark.parametrize("vdtype", ["int8", "int32", "int64"])
def test_integer_m2_within_8u_of_the_sum_of_squares(gx, shim, vdtype):  # noqa: F811
    """one rounding each of sum x^2, sum x, the product, the quotient and the difference, each at most u S2* since
    (sum x)^2 / c <= sum x^2; VAR and STD are that M2 / (c - ddof) and its square root.  M2 >= 0 wherever (sum x)^2 < 2^53 as
    well: the product is exact then and the correctly rounded quotient cannot pass sum x^2.  (Beyond that a constant group can
    come out one rounding error below 0 -- int64 2^20 + 1 in 4097 rows does; the integer arithmetic is the reference's.)"""
    Column, ops = gx
    vals, keys, vv, m2, s2, c, exact_square = _integers(vdtype)
    for ddof in (0, 1, 2):
        k, var, std, gm2, cv = ops.groupby_var_std(Column.from_numpy(keys), Column.from_numpy(vals, vv), ddof=ddof)
        np.testing.assert_array_equal(cv.to_numpy(), c)
        got = gm2.to_numpy()
        assert _valid(gm2).all()
        _check_integer_m2(got, m2, s2, exact_square, f"{vdtype} ops")
        ok = c - ddof > 0
        np.testing.assert_array_equal(_valid(var), ok)
        np.testing.assert_array_equal(_valid(std), ok)
        np.testing.assert_array_equal(var.to_numpy()[ok], got[ok] / (c[ok] - ddof))
        with np.errstate(invalid="ignore"):
            np.testing.assert_array_equal(std.to_numpy()[ok], np.sqrt(got[ok] / (c[ok] - ddof)))
    for force_sort in (0, 1):
        _, _, got, valid = _cpp_aggregate(shim, keys, None, vals, vv, M2, 0, 0, 0, force_sort)
        assert valid.all()
        _check_integer_m2(got, m2, s2, exact_square, f"{vdtype} cudf::groupby force_sort={force_sort}")


# ---------------------------------------------------------------------------------------------------------------------
# the kernels through the C ABI
# ---------------------------------------------------------------------------------------------------------------------
GUARD = 0x5A5A5A5A
GROUPS = [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 4096 * 256 + 65]  # the last: the second trip of the launch's capped grid


def _finaliser_inputs(G, variant):
    rng = np.random.default_rng(G)
    i = np.arange(G)
    cnt = (3 + rng.integers(0, 6, G)).astype(np.int32)
    # counts 0 / 1 / 2 (null for some mode and ddof) on both sides of the word edges: bit 31 and bit 0 together, or either alone
    word = i // 32
    cnt[(i % 32 == 31) & (word % 3 != 2)] = rng.integers(0, 3, G)[(i % 32 == 31) & (word % 3 != 2)]
    cnt[(i % 32 == 0) & (word % 3 != 0)] = rng.integers(0, 3, G)[(i % 32 == 0) & (word % 3 != 0)]
    cnt[i % 64 == 33] = 2
    if variant == "int64":
        sm = rng.integers(-10**6, 10**6, G)
        ss = rng.integers(0, 10**12, G)                # also below sum^2 / count: a negative M2 and a NaN STD, as NumPy's
    elif variant == "float64":
        sm = rng.standard_normal(G) * 1e3
        ss = rng.random(G) * 1e6
    else:                                              # the sum of the centred squares: M2 itself
        sm = None
        ss = rng.random(G) * 10.0 ** rng.integers(-30, 30, G)
        ss[::7] = 0.0
        ss[3::11] = -ss[3::11]                         # raised to 0
        ss[5::13] = np.nan                             # kept
        ss[6::17] = np.inf
        ss[8::19] = -0.0
    return cnt, ss, sm


@pytest.mark.parametrize("variant", ["int64", "float64", "centred"])
@pytest.mark.parametrize("G", GROUPS)
def test_var_from_sums_bit_for_bit(gx, G, variant):
    import torch
    from cudf_amd import _lib as L
    from cudf_amd.column import unpack_mask
    _, ops = gx
    cnt, ss, sm = _finaliser_inputs(G, variant)
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    dcnt, dss, dsm = dev(cnt), dev(ss), (dev(sm) if sm is not None else None)
    words = (G + 31) // 32
    c = cnt.astype(np.float64)
    with np.errstate(all="ignore"):
        if variant == "centred":
            m2 = np.where(ss < 0, 0.0, ss)
        else:
            m2 = ss.astype(np.float64) - sm.astype(np.float64) * sm.astype(np.float64) / c
    for mode in (0, 1, 2):
        for ddof in (0, 1, 2) if mode else (1,):
            out = torch.full((G,), -7.0, dtype=torch.float64, device="cuda")
            mask = torch.full((words + 1,), GUARD, dtype=torch.int32, device="cuda")
            nulls = torch.full((1,), -1, dtype=torch.int64, device="cuda")
            L.check(L.lib.gx_var_from_sums(L.INT64 if variant == "int64" else L.FLOAT64, ops.ptr(dss), ops.ptr(dsm), ops.ptr(dcnt), G, ddof, mode,
                                           ops.ptr(out), ops.ptr(mask), ops.ptr(nulls), ops.stream_ptr()), "gx_var_from_sums")
            hmask = mask.cpu().numpy().view(np.uint32)
            assert hmask[words] == GUARD, "the word behind the mask was written"
            valid = unpack_mask(hmask[:words], G)
            with np.errstate(all="ignore"):
                if mode == 0:
                    want_valid, want = np.ones(G, bool), np.where(cnt > 0, m2, 0.0)
                else:
                    want_valid = (cnt > 0) & (cnt - ddof > 0)
                    want = m2 / (c - ddof)
                    want = np.sqrt(want) if mode == 2 else want
            np.testing.assert_array_equal(valid, want_valid)
            assert int(nulls.item()) == int((~want_valid).sum())
            got = out.cpu().numpy()
            nan = np.isnan(want)
            np.testing.assert_array_equal(np.isnan(got)[want_valid], nan[want_valid])
            sel = want_valid & ~nan
            np.testing.assert_array_equal(got[sel].view(np.int64), want[sel].view(np.int64))  # bit for bit: -0.0 stays -0.0


@pytest.mark.parametrize("n", [1, 255, 2049, 16384 * 256 + 77])  # the last: the second trip of the launch's capped grid
def test_square_centered_bit_for_bit(gx, n):
    import torch
    from cudf_amd import _lib as L
    _, ops = gx
    rng = np.random.default_rng(n)
    G = 37
    x = 1e8 + rng.standard_normal(n)
    x[::101] = np.nan
    x[1::103] = np.inf
    gid = rng.integers(0, G, n).astype(np.int32)
    gid[::13] = -(2**31)   # no group (a null key): 0
    gid[1::29] = -1
    gid[2::31] = G         # outside the groups: 0, nothing read
    mean = 1e8 + rng.standard_normal(G)
    mean[5] = np.inf
    dx, dg, dm = torch.from_numpy(x).cuda(), torch.from_numpy(gid).cuda(), torch.from_numpy(mean).cuda()
    out = torch.full((n + 1,), -7.0, dtype=torch.float64, device="cuda")
    L.check(L.lib.gx_square_centered(ops.ptr(dx), ops.ptr(dg), ops.ptr(dm), n, G, ops.ptr(out), ops.stream_ptr()), "gx_square_centered")
    got = out.cpu().numpy()
    assert got[n] == -7.0, "the element behind the output was written"
    inside = (gid >= 0) & (gid < G)
    with np.errstate(invalid="ignore"):
        d = x - mean[np.where(inside, gid, 0)]
        want = np.where(inside, d * d, 0.0)
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got[:n]), nan)
    np.testing.assert_array_equal(got[:n][~nan].view(np.int64), want[~nan].view(np.int64))


@pytest.mark.parametrize("dtype", route.DTYPES)
def test_square_dtype_routes(gx, dtype):
    """gx_square picks <value type, INT64 or the float's own type> from the dtype: one wave and a tail row of the values that tell a
    wrong instantiation from the right one (tests/route_values.py).  Integers are shifted so that no square passes 2^63: int64
    arithmetic, as in the kernel.  (Not told apart: INT64 from UINT64 -- the squares agree mod 2^64.)"""
    from cudf_amd import _lib as L
    Column, ops = gx
    v = route.route_values(dtype, seed=4)
    dt = v.dtype
    if dt.kind in "iu" and dt.itemsize >= 4:
        v = v >> (32 if dt.itemsize == 8 else 1)       # arithmetic for the signed types: negative values stay negative
        if dt == np.uint32:
            v[64] = 2**31 + 5                            # as INT32 it would be -(2^31 - 5): another square
    col = Column.from_numpy(v)
    out = Column.empty(dt if dt.kind == "f" else np.int64, len(v))
    L.check(L.lib.gx_square(col.gx, col.data_ptr, len(v), out.data_ptr, ops.stream_ptr()), "gx_square")
    with np.errstate(invalid="ignore", over="ignore"):
        want = v * v if dt.kind == "f" else v.astype(np.int64) * v.astype(np.int64)
    np.testing.assert_array_equal(out.to_numpy(), want)
