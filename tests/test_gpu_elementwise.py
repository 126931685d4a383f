"""GPU: cudf::binary_operation / unary_operation / cast -- ops.binary_operation, ops.unary_operation, ops.cast, the Column operators
and the entry points under them (cudf_amd/csrc/gx_elementwise.hip), plus the C++ surface (tests/cpp/cudf_binaryop_tests).
The reference is NumPy on the host.  The value model is out = cast<Out>(f(cast<C>(lhs), cast<C>(rhs))) with C the common type of
C++ (class_of below), NOT np.result_type; expected values are computed by casting both arrays to C first.  Valid rows are compared
bit for bit; two NaNs count as equal whatever their sign and payload (IEEE 754 leaves both to the implementation, and the host's
default NaN differs from the device's).  Row counts come from T = gx_elementwise_tile_rows()."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = ["int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float32", "float64", "bool"]
INTS = DTYPES[:8]
FLOATS = ["float32", "float64"]
BEGIN_BITS = (0, 1, 31, 33)
BIG = 2**22 + 4097
CMP = {"EQUAL": np.equal, "NOT_EQUAL": np.not_equal, "LESS": np.less, "GREATER": np.greater, "LESS_EQUAL": np.less_equal,
       "GREATER_EQUAL": np.greater_equal}


@pytest.fixture(scope="module")
def gx():
    import cudf_amd
    from cudf_amd import Column, ops
    return cudf_amd, Column, ops


@pytest.fixture(scope="module")
def T(gx):
    return int(gx[0]._lib.lib.gx_elementwise_tile_rows())


@pytest.fixture(scope="module")
def ROWS(T):
    return (0, 1, 31, 32, 33, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17)


# ------------------------------------------------------------------------------------------------ the host model
_CLS_ORDER = ["int32", "uint32", "int64", "uint64", "float32", "float64"]


def class_of(*dts):
    """the type the usual arithmetic conversions of C++ give: below 32 bits (and bool) -> int32, then the larger class"""
    best = 0
    for dt in dts:
        dt = np.dtype(dt)
        best = max(best, _CLS_ORDER.index(dt.name) if dt.name in _CLS_ORDER else 0)
    return np.dtype(_CLS_ORDER[best])


def cast(a, dt):
    """static_cast on in-range values: to bool x != 0, float -> integer truncates, integer -> narrower integer wraps"""
    dt = np.dtype(dt)
    with np.errstate(all="ignore"):
        if dt == np.bool_:
            return np.asarray(a) != 0
        return np.asarray(a).astype(dt)


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same(got, want):
    """bit for bit; NaN == NaN"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    eq = bits_of(got) == bits_of(want)
    if got.dtype.kind == "f":
        eq |= np.isnan(got) & np.isnan(want)
    return eq


def assert_same(got, want, what="", valid=None):
    eq = same(got, want)
    if valid is not None:
        eq = eq | ~valid
    if not eq.all():
        i = int(np.flatnonzero(~eq)[0])
        raise AssertionError(f"{what}: {int((~eq).sum())} rows differ, first at {i}: got {got[i]!r}, want {want[i]!r}")


def trunc_div(x, y):
    q = x // y
    if x.dtype.kind == "i":
        q = q + ((x % y != 0) & ((x < 0) != (y < 0)))
    return q.astype(x.dtype)


def ref_binop(op, x, y, lhs_dt=None):
    """f on two arrays already cast to C; the result in C (a truth value as bool), TRUE_DIV / POW as the kernel carries them"""
    C = x.dtype
    with np.errstate(all="ignore"):
        if op == "ADD":
            return x + y
        if op == "SUB":
            return x - y
        if op == "MUL":
            return x * y
        if op in CMP:
            return CMP[op](x, y)
        if op == "DIV":
            return x / y if C.kind == "f" else trunc_div(x, y)
        if op == "TRUE_DIV":
            return x.astype(np.float64) / y.astype(np.float64)
        if op == "MOD":
            return np.fmod(x, y)
        if op == "FLOOR_DIV":
            return np.floor_divide(x, y)
        if op == "PYMOD":
            return np.mod(x, y)
        if op == "PMOD":
            if C.kind != "f":
                return np.mod(x, y)
            r = np.fmod(x, y)
            return np.where(r < 0, np.fmod(r + y, y), r)
        if op == "LOGICAL_AND":
            return (x != 0) & (y != 0)
        if op == "LOGICAL_OR":
            return (x != 0) | (y != 0)
        if op == "BITWISE_AND":
            return x & y
        if op == "BITWISE_OR":
            return x | y
        if op == "BITWISE_XOR":
            return x ^ y
        if op == "SHIFT_LEFT":
            return x << y
        if op == "SHIFT_RIGHT":
            return x >> y
        if op == "SHIFT_RIGHT_UNSIGNED":
            w = np.dtype(lhs_dt).itemsize * 8
            u = np.dtype(f"uint{C.itemsize * 8}")
            ux = x.astype(u) & u.type((1 << w) - 1) if w < C.itemsize * 8 else x.astype(u)
            return (ux >> y.astype(u)).astype(C)
    raise KeyError(op)


def expected(op, a, b, out_dt):
    C = class_of(a.dtype, b.dtype)
    return cast(ref_binop(op, cast(a, C), cast(b, C), a.dtype), out_dt)


def values(rng, dt, n, small=False, nonneg=False):
    """n values of dt over its whole width with the extremes among them; small: |v| <= 50 (halves for floats), nonneg: none below 0"""
    dt = np.dtype(dt)
    if dt == np.bool_:
        return rng.integers(0, 2, n).astype(np.bool_)
    if small:
        lo = 0 if dt.kind == "u" or nonneg else -50
        v = rng.integers(lo * 2, 101, n) / 2
        return v.astype(dt) if dt.kind == "f" else np.trunc(v).astype(dt)
    if dt.kind == "f":
        v = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(dt)
        return v
    info = np.iinfo(dt)
    v = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    edge = np.array([info.min, info.max, 0, 1, info.max - 1, info.min + 1], dtype=dt)
    k = min(n, len(edge))
    v[rng.permutation(n)[:k]] = edge[:k]
    return v


def safe_divisor(x, y):
    """nonzero, and never the INT_MIN / -1 pair"""
    y = y.copy()
    if y.dtype == np.bool_:
        y[:] = True
        return y
    y[y == 0] = 1
    if y.dtype.kind == "i":
        C = class_of(x.dtype, y.dtype)
        if C.kind == "i":
            y[(cast(x, C) == np.iinfo(C).min) & (y == -1)] = 1
    return y


SPECIALS = [0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 0.1, -0.1, 3.0, -3.0, 2.5, -7.5, 1e30, -1e30]


def float_inputs(rng, dt, n):
    """every ordered pair of the specials (signed zeros, infinities, NaN, denormals, both signs), then random values"""
    dt = np.dtype(dt)
    tiny = np.finfo(dt).smallest_subnormal
    sp = np.array(SPECIALS + [tiny, -tiny, 3 * tiny, np.finfo(dt).tiny, np.finfo(dt).max, -np.finfo(dt).max], dtype=dt)
    a, b = (m.ravel() for m in np.meshgrid(sp, sp, indexing="ij"))
    m = max(n - len(a), 0)
    x = np.concatenate([a, values(rng, dt, m)])[:n]
    y = np.concatenate([b, values(rng, dt, m) * dt.type(0.37)])[:n]
    return x.astype(dt), y.astype(dt)


def run(gx, op, a, b, out_dt, av=None, bv=None):
    """ops.binary_operation on host arrays (or scalars); returns the result Column"""
    _, Column, ops = gx
    lhs = Column.from_numpy(a, av) if isinstance(a, np.ndarray) else a
    rhs = Column.from_numpy(b, bv) if isinstance(b, np.ndarray) else b
    return ops.binary_operation(lhs, rhs, op, out_dt)


# ------------------------------------------------------------------------------------------------ same-type arithmetic
@pytest.mark.parametrize("dt", DTYPES)
def test_same_type_arithmetic_and_comparisons_every_row_count(gx, ROWS, dt):
    """ADD / SUB / MUL / DIV / MOD and the six comparisons on two columns of one dtype at every row count of the set; integers hold
    the type's extremes and wrap, divisors are nonzero and never INT_MIN / -1; floats are bit-exact (no fast-math: the device's
    divide is correctly rounded)"""
    _, Column, ops = gx
    rng = np.random.default_rng(DTYPES.index(dt))
    for n in ROWS:
        if np.dtype(dt).kind == "f":
            a, b = float_inputs(rng, dt, n)
            d = b
        else:
            a, b = values(rng, dt, n), values(rng, dt, n)
            d = safe_divisor(a, b)
        ca, cb, cd = Column.from_numpy(a), Column.from_numpy(b), Column.from_numpy(d)
        for op in ("ADD", "SUB", "MUL"):
            got = ops.binary_operation(ca, cb, op, dt)
            assert got.size == n and got.mask is None and got.null_count == 0
            assert_same(got.to_numpy(), expected(op, a, b, dt), f"{op} {dt} n={n}")
        for op in ("DIV", "MOD"):
            assert_same(ops.binary_operation(ca, cd, op, dt).to_numpy(), expected(op, a, d, dt), f"{op} {dt} n={n}")
        for op in CMP:
            got = ops.binary_operation(ca, cb, op, np.bool_)
            assert got.dtype == np.bool_
            assert_same(got.to_numpy(), expected(op, a, b, np.bool_), f"{op} {dt} n={n}")


def test_grid_stride_second_trip_and_a_large_column(gx, T):
    """one row count just above grid cap x T (the grid-stride loop takes a second trip) on int8, whose tiles are the fewest bytes,
    with both bitmaps; 2^22 + 4097 rows once on int64"""
    cudf_amd, Column, ops = gx
    cap = int(cudf_amd._lib.lib.gx_elementwise_grid_cap())
    rng = np.random.default_rng(99)
    for dt, n in (("int8", cap * T + 37), ("int64", BIG)):
        a, b = values(rng, dt, n), values(rng, dt, n)
        av, bv = rng.random(n) < 0.8, rng.random(n) < 0.8
        got = run(gx, "ADD", a, b, dt, av, bv)
        valid = av & bv
        assert got.null_count == int((~valid).sum())
        assert np.array_equal(got.valid_numpy(), valid)
        assert_same(got.to_numpy(), expected("ADD", a, b, dt), f"ADD {dt} n={n}", valid)
        got = run(gx, "LESS", a, b, np.bool_)
        assert got.mask is None
        assert_same(got.to_numpy(), expected("LESS", a, b, np.bool_), f"LESS {dt} n={n}")


# ------------------------------------------------------------------------------------------------ floats: the division family
@pytest.mark.parametrize("dt", FLOATS)
def test_float_mod_pmod_pymod_floor_div_sqrt_bit_exact(gx, T, dt):
    """MOD against np.fmod, PMOD against r = fmod(x, y); r < 0: fmod(r + y, y), PYMOD against np.mod, FLOOR_DIV against
    np.floor_divide, SQRT against np.sqrt: signed zeros, infinities, NaN, denormals and both signs of divisor in every pairing"""
    _, Column, ops = gx
    rng = np.random.default_rng(5)
    n = 3 * T + 17
    a, b = float_inputs(rng, dt, n)
    ca, cb = Column.from_numpy(a), Column.from_numpy(b)
    for op in ("MOD", "PMOD", "PYMOD", "FLOOR_DIV", "DIV", "TRUE_DIV"):
        out = np.float64 if op == "TRUE_DIV" else dt
        assert_same(ops.binary_operation(ca, cb, op, out).to_numpy(), expected(op, a, b, out), f"{op} {dt}")
    with np.errstate(all="ignore"):
        assert_same(ops.unary_operation(ca, "SQRT").to_numpy(), np.sqrt(a), f"SQRT {dt}")
        assert_same(ops.unary_operation(Column.from_numpy(np.abs(b)), "SQRT").to_numpy(), np.sqrt(np.abs(b)), f"SQRT {dt}")


# ------------------------------------------------------------------------------------------------ mixed types
@pytest.mark.parametrize("out_dt", ["class", "int8", "bool", "float64", "uint16"])
def test_mixed_types_every_ordered_pair_add_and_less(gx, out_dt):
    """every ordered pair of the 11 dtypes under ADD and LESS; expected = both arrays cast to the compute class C, the operator
    there, then the cast to the output dtype (C itself, a narrower type, BOOL8, float64).  Where C is a float class the values
    are small halves, so that the cast of the result to an integer output stays in range (out of range is unspecified)"""
    _, Column, ops = gx
    rng = np.random.default_rng(17)
    n = 333
    for ld, rd in itertools.product(DTYPES, repeat=2):
        C = class_of(ld, rd)
        small = C.kind == "f"
        o = C if out_dt == "class" else np.dtype(out_dt)
        nonneg = small and o.kind == "u"     # a negative float sum into an unsigned output would be out of range
        a, b = values(rng, ld, n, small, nonneg), values(rng, rd, n, small, nonneg)
        ca, cb = Column.from_numpy(a), Column.from_numpy(b)
        assert_same(ops.binary_operation(ca, cb, "ADD", o).to_numpy(), expected("ADD", a, b, o), f"ADD {ld} {rd} -> {o}")
        assert_same(ops.binary_operation(ca, cb, "LESS", o).to_numpy(), expected("LESS", a, b, o), f"LESS {ld} {rd} -> {o}")


def test_mixed_types_pinned_cases(gx):
    """int32(-1) < uint32(1) is false (compared as uint32); uint32 + uint32 wraps at 2^32 before it is widened to int64;
    int64 + uint64 computes in uint64; int8 + int8 computes in int32"""
    got = run(gx, "LESS", np.array([-1, 0], np.int32), np.array([1, 1], np.uint32), np.bool_).to_numpy()
    assert got.tolist() == [False, True]
    got = run(gx, "ADD", np.array([2**32 - 1, 5], np.uint32), np.array([2, 6], np.uint32), np.int64).to_numpy()
    assert got.tolist() == [1, 11]
    got = run(gx, "ADD", np.array([-1], np.int64), np.array([0], np.uint64), np.uint64).to_numpy()
    assert got.tolist() == [2**64 - 1]
    got = run(gx, "LESS", np.array([-1], np.int64), np.array([1], np.uint64), np.bool_).to_numpy()
    assert got.tolist() == [False]
    got = run(gx, "ADD", np.array([100, -100], np.int8), np.array([100, -100], np.int8), np.int32).to_numpy()
    assert got.tolist() == [200, -200]
    got = run(gx, "MUL", np.array([2**31 - 1], np.int32), np.array([2], np.int32), np.int64).to_numpy()
    assert got.tolist() == [-2]                          # wraps in int32, then widens
    got = run(gx, "ADD", np.array([3, 0], np.uint8), np.array([1, 0], np.bool_), np.bool_).to_numpy()
    assert got.tolist() == [True, False]                 # a store to BOOL8 writes x != 0


# ------------------------------------------------------------------------------------------------ integers
@pytest.mark.parametrize("dt", INTS)
def test_integer_floor_div_and_pymod_against_python_operators(gx, T, dt):
    """FLOOR_DIV against //, PYMOD and PMOD against %, all four sign combinations, magnitudes up to 2^62 for int64"""
    rng = np.random.default_rng(23)
    n = T + 33
    info = np.iinfo(dt)
    top = min(info.max, 2**62)
    lo = 0 if info.min == 0 else -top
    a = rng.integers(lo, top, n, dtype=dt, endpoint=True)
    b = rng.integers(lo, top, n, dtype=dt, endpoint=True)
    small = rng.integers(lo if lo == 0 else -9, 9, n, dtype=dt, endpoint=True)
    for x, y in ((a, b), (a, small)):
        y = safe_divisor(x, y)
        for s1, s2 in itertools.product((1, -1), repeat=2) if lo < 0 else ((1, 1),):
            xx = (np.abs(x) * s1).astype(dt)
            yy = (np.abs(y) * s2).astype(dt)
            want_q = np.array([int(p) // int(q) for p, q in zip(xx.tolist(), yy.tolist())]).astype(dt)
            want_r = np.array([int(p) % int(q) for p, q in zip(xx.tolist(), yy.tolist())]).astype(dt)
            assert_same(run(gx, "FLOOR_DIV", xx, yy, dt).to_numpy(), want_q, f"FLOOR_DIV {dt}")
            assert_same(run(gx, "PYMOD", xx, yy, dt).to_numpy(), want_r, f"PYMOD {dt}")
            assert_same(run(gx, "PMOD", xx, yy, dt).to_numpy(), want_r, f"PMOD {dt}")


def test_shift_right_unsigned_is_logical_on_the_operands_own_width(gx):
    for dt in ("int8", "int32", "int64"):
        w = np.dtype(dt).itemsize * 8
        x = np.array([-1, np.iinfo(dt).min, -2, np.iinfo(dt).min + 5, 100, -100], dtype=dt)
        for s in (1, 3, w - 1, 0):
            y = np.full(len(x), s, dtype=dt)
            want = (x.view(f"uint{w}") >> np.array(s, dtype=f"uint{w}")).view(dt)
            assert_same(run(gx, "SHIFT_RIGHT_UNSIGNED", x, y, dt).to_numpy(), want, f"SHIFT_RIGHT_UNSIGNED {dt} by {s}")
            assert_same(run(gx, "SHIFT_RIGHT", x, y, dt).to_numpy(), x >> y, f"SHIFT_RIGHT {dt} by {s}")
            assert_same(run(gx, "SHIFT_LEFT", x, y, dt).to_numpy(), x << y, f"SHIFT_LEFT {dt} by {s}")
    assert run(gx, "SHIFT_RIGHT_UNSIGNED", np.array([-1], np.int8), np.array([1], np.int8), np.int8).to_numpy().tolist() == [127]
    # an int32 operand beside an int64 shift count: the class is int64, the operand's own width still 32
    got = run(gx, "SHIFT_RIGHT_UNSIGNED", np.array([-1], np.int32), np.array([1], np.int64), np.int64).to_numpy()
    assert got.tolist() == [2**31 - 1]


@pytest.mark.parametrize("dt", INTS + ["bool"])
def test_bitwise_and_logical_operators(gx, T, dt):
    rng = np.random.default_rng(29)
    n = T + 5
    a, b = values(rng, dt, n), values(rng, dt, n)
    a[::7] = 0
    for op in ("BITWISE_AND", "BITWISE_OR", "BITWISE_XOR"):
        assert_same(run(gx, op, a, b, dt).to_numpy(), expected(op, a, b, dt), f"{op} {dt}")
    for op in ("LOGICAL_AND", "LOGICAL_OR"):
        assert_same(run(gx, op, a, b, np.bool_).to_numpy(), expected(op, a, b, np.bool_), f"{op} {dt}")


@pytest.mark.parametrize("dt", INTS)
def test_int_pow_wraps_and_a_negative_exponent_gives_zero(gx, dt):
    rng = np.random.default_rng(31)
    info = np.iinfo(dt)
    C = class_of(dt)
    bits = C.itemsize * 8
    n = 4099
    base = values(rng, dt, n)
    base[:64] = rng.integers(max(info.min, -3), 4, 64)
    e_lo = 0 if info.min == 0 else -4
    exp = rng.integers(e_lo, 40, n).astype(dt)
    exp[:8] = 0
    want = []
    for p, q in zip(base.tolist(), exp.tolist()):
        r = 0 if q < 0 else pow(p, q, 1 << bits)          # wraps modulo 2^width of C, then the cast to dt wraps again
        want.append(r)
    want = np.array(want, dtype=np.uint64).astype(dt)
    assert_same(run(gx, "INT_POW", base, exp, dt).to_numpy(), want, f"INT_POW {dt}")


# ------------------------------------------------------------------------------------------------ POW
# The largest distance measured on an MI355X against the references below over the 300 000 sampled rows: float64 1 ulp,
# float32 1 ulp.  The assertion allows twice that.
POW_MEASURED_ULP = {"float64": 1, "float32": 1}


def ulp_distance(a, b):
    i = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return np.abs(a.view(i).astype(np.int64) - b.view(i).astype(np.int64))      # same sign here: positive results


@pytest.mark.parametrize("dt", FLOATS)
def test_pow_accuracy(gx, dt):
    """bases in (0, 100], exponents in [-8, 8]; float64 against np.power in np.longdouble rounded to float64, float32 against
    float64 rounded to float32; the largest ulp distance is printed and asserted at twice the measured value"""
    rng = np.random.default_rng(37)
    n = 300_000
    x = (100.0 * (1.0 - rng.random(n))).astype(dt)
    y = rng.uniform(-8, 8, n).astype(dt)
    wide = np.longdouble if dt == "float64" else np.float64
    want = np.power(x.astype(wide), y.astype(wide)).astype(dt)
    got = run(gx, "POW", x, y, dt).to_numpy()
    ok = np.isfinite(want) & (want > 0)
    worst = int(ulp_distance(got[ok], want[ok]).max())
    print(f"POW {dt}: largest distance {worst} ulp over {int(ok.sum())} rows")
    assert worst <= 16, "a defect to investigate, not a tolerance"
    assert worst <= 2 * POW_MEASURED_ULP[dt]


@pytest.mark.parametrize("dt", FLOATS)
def test_pow_special_cases_bit_exact(gx, dt):
    inf, nan = np.inf, np.nan
    cases = [(2.0, 0.0, 1.0), (-3.5, 0.0, 1.0), (nan, 0.0, 1.0), (inf, 0.0, 1.0), (0.0, 0.0, 1.0),          # x ** 0
             (1.0, 5.5, 1.0), (1.0, -inf, 1.0), (1.0, nan, 1.0),                                             # 1 ** y
             (0.0, 3.0, 0.0), (0.0, 0.5, 0.0), (-0.0, 3.0, -0.0), (-0.0, 2.0, 0.0),                          # 0 ** positive
             (inf, 2.0, inf), (inf, -2.0, 0.0), (-inf, 3.0, -inf), (-inf, 2.0, inf), (2.0, inf, inf), (2.0, -inf, 0.0),
             (0.5, inf, 0.0), (0.5, -inf, inf),
             (-2.0, 3.0, -8.0), (-2.0, 2.0, 4.0), (-2.0, -2.0, 0.25), (-3.0, 5.0, -243.0), (-1.0, 101.0, -1.0), (-10.0, 4.0, 10000.0),
             (-2.0, 0.5, nan)]
    x = np.array([c[0] for c in cases], dtype=dt)
    y = np.array([c[1] for c in cases], dtype=dt)
    want = np.array([c[2] for c in cases], dtype=dt)
    assert_same(run(gx, "POW", x, y, dt).to_numpy(), want, f"POW {dt}")
    # integer operands: pow(double(x), double(y))
    got = run(gx, "POW", np.array([2, -3, 7], np.int32), np.array([10, 3, 0], np.int32), np.float64).to_numpy()
    assert got.tolist() == [1024.0, -27.0, 1.0]


# ------------------------------------------------------------------------------------------------ validity
def truth_valid(op, lv, rv, xt, yt):
    """the validity rules row by row (the model of tests/test_elementwise_host.py)"""
    if op in ("NULL_EQUALS", "NULL_NOT_EQUALS"):
        return np.ones(len(lv), dtype=bool)
    if op in ("NULL_MAX", "NULL_MIN"):
        return lv | rv
    if op == "NULL_LOGICAL_AND":
        return (lv & rv) | (lv & ~xt) | (rv & ~yt)
    if op == "NULL_LOGICAL_OR":
        return (lv & rv) | (lv & xt) | (rv & yt)
    return lv & rv


def null_op_values(op, a, b, lv, rv, out_dt):
    C = class_of(a.dtype, b.dtype)
    x, y = cast(a, C), cast(b, C)
    both = lv & rv
    if op == "NULL_EQUALS":
        r = np.where(both, x == y, lv == rv)
    elif op == "NULL_NOT_EQUALS":
        r = np.where(both, x != y, lv != rv)
    elif op == "NULL_MAX":
        r = np.where(both, np.where(x < y, y, x), np.where(lv, x, y))
    elif op == "NULL_MIN":
        r = np.where(both, np.where(y < x, y, x), np.where(lv, x, y))
    elif op == "NULL_LOGICAL_AND":
        r = (~lv | (x != 0)) & (~rv | (y != 0))
    else:
        r = (lv & (x != 0)) | (rv & (y != 0))
    return cast(r, out_dt)


def check_column(got, want_values, want_valid, what=""):
    nulls = int((~want_valid).sum())
    assert got.null_count == nulls, (what, got.null_count, nulls)
    if nulls == 0:
        assert got.mask is None, what
    else:
        assert got.mask is not None and np.array_equal(got.valid_numpy(), want_valid), what
    assert_same(got.to_numpy(), want_values, what, want_valid)


@pytest.mark.parametrize("which", ["lhs", "rhs", "both"])
def test_nullable_operands(gx, ROWS, which):
    """a bitmap on lhs, on rhs, on both, validity 0.8, every row count: the output bit is the AND, the null count is counted"""
    rng = np.random.default_rng(41)
    for n in ROWS:
        a, b = values(rng, "int32", n), values(rng, "float64", n, True)
        av = rng.random(n) < 0.8 if which in ("lhs", "both") else None
        bv = rng.random(n) < 0.8 if which in ("rhs", "both") else None
        valid = (av if av is not None else np.ones(n, bool)) & (bv if bv is not None else np.ones(n, bool))
        for op, out in (("ADD", np.float64), ("LESS", np.bool_), ("TRUE_DIV", np.float64)):
            y = safe_divisor(a, b) if op == "TRUE_DIV" else b
            check_column(run(gx, op, a, y, out, av, bv), expected(op, a, y, out), valid, f"{op} {which} n={n}")


def test_all_null_and_no_null_results(gx, T):
    rng = np.random.default_rng(43)
    n = 2 * T + 3
    a, b = values(rng, "int16", n), values(rng, "int16", n)
    none, every = np.zeros(n, bool), np.ones(n, bool)
    got = run(gx, "ADD", a, b, np.int16, none, every)
    assert got.null_count == n and not got.valid_numpy().any()
    got = run(gx, "ADD", a, b, np.int16, none, none)
    assert got.null_count == n and not got.valid_numpy().any()
    # masks present, nothing null: the count is 0 and the mask is dropped
    got = run(gx, "ADD", a, b, np.int16, every, every)
    assert got.null_count == 0 and got.mask is None
    assert_same(got.to_numpy(), expected("ADD", a, b, np.int16))
    # one null row in the last word
    last = every.copy()
    last[-1] = False
    check_column(run(gx, "SUB", a, b, np.int16, last, every), expected("SUB", a, b, np.int16), last, "one null")


def raw_binary_op(gx, op, a, av, abit, b, bv, bbit, out_dt, want_valid=True):
    """gx_binary_op through the ABI with the operands' bitmaps at their own begin bits, noise in front of and behind the rows;
    returns (values, validity as bool array or None, null count)"""
    import torch
    cudf_amd, Column, _ = gx
    L = cudf_amd._lib
    from cudf_amd.column import ptr, stream_ptr, gx_dtype, pack_mask, unpack_mask, bitmask_words
    n = len(a)
    rng = np.random.default_rng(abit * 64 + bbit)

    def mask(v, bit):
        if v is None:
            return None
        buf = rng.integers(0, 2, bit + n + 40).astype(bool)
        buf[bit:bit + n] = v
        return torch.from_numpy(pack_mask(buf).view(np.int32).copy()).cuda()

    ca, cb = Column.from_numpy(a), Column.from_numpy(b)
    ma, mb = mask(av, abit), mask(bv, bbit)
    out = Column.empty(out_dt, n)
    words = torch.full((bitmask_words(n) + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") if want_valid else None
    nulls = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    rc = L.lib.gx_binary_op(L.BINOP[op], ca.gx, ca.data_ptr, ptr(ma), abit, None, 0, cb.gx, cb.data_ptr, ptr(mb), bbit, None, 0, n,
                            gx_dtype(out_dt), out.data_ptr, ptr(words), ptr(nulls), stream_ptr())
    assert rc == 0
    if words is None:
        return out.to_numpy(), None, int(nulls.item())
    w = words.cpu().numpy().view(np.uint32)
    used = (n + 31) // 32
    assert (w[used:] == 0x5A5A5A5A).all()               # nothing behind the (n + 31) / 32 words is written
    bits = np.unpackbits(w[:used].view(np.uint8), bitorder="little")
    assert not bits[n:].any()                            # padding bits are 0
    return out.to_numpy(), bits[:n].astype(bool), int(nulls.item())


NULL_OPS = ("NULL_EQUALS", "NULL_NOT_EQUALS", "NULL_MAX", "NULL_MIN", "NULL_LOGICAL_AND", "NULL_LOGICAL_OR")


@pytest.mark.parametrize("op", ("ADD", "FLOOR_DIV", "TRUE_DIV") + NULL_OPS)
def test_validity_at_independent_begin_bits_through_the_abi(gx, T, op):
    """both bitmaps at begin bits 0 / 1 / 31 / 33 independently, every operator family and every NULL_* operator against the host
    model; every word written, padding bits 0, the null count as an integer; widths 1, 4 and 8 bytes (16, 4 and 2 rows per access)"""
    rng = np.random.default_rng(47)
    for dt, n in (("int8", T + 45), ("int32", 1000), ("int64", 3 * 64 + 7)):
        a, b = values(rng, dt, n), values(rng, dt, n)
        a[::3] = 0
        b[::5] = 0
        if op in ("FLOOR_DIV", "TRUE_DIV"):
            b = safe_divisor(a, b)
        av, bv = rng.random(n) < 0.8, rng.random(n) < 0.8
        out = np.dtype(np.bool_) if "LOGICAL" in op or "EQUALS" in op else np.dtype(np.float64 if op == "TRUE_DIV" else dt)
        for abit, bbit in itertools.product(BEGIN_BITS, repeat=2):
            got, valid, nulls = raw_binary_op(gx, op, a, av, abit, b, bv, bbit, out)
            want_valid = truth_valid(op, av, bv, a != 0, b != 0)
            want = null_op_values(op, a, b, av, bv, out) if op in NULL_OPS else expected(op, a, b, out)
            assert np.array_equal(valid, want_valid), (op, dt, abit, bbit)
            assert nulls == int((~want_valid).sum()), (op, dt, abit, bbit)
            assert_same(got, want, f"{op} {dt} bits {abit} {bbit}", want_valid)
        # one side without a bitmap
        got, valid, nulls = raw_binary_op(gx, op, a, None, 0, b, bv, 33, out)
        every = np.ones(n, bool)
        want_valid = truth_valid(op, every, bv, a != 0, b != 0)
        assert np.array_equal(valid, want_valid) and nulls == int((~want_valid).sum())
    # out_valid == NULL: no bitmap is read or written, the count stays 0
    got, valid, nulls = raw_binary_op(gx, op, a, None, 0, b, None, 0, out, want_valid=False)
    every = np.ones(len(a), bool)
    want = null_op_values(op, a, b, every, every, out) if op in NULL_OPS else expected(op, a, b, out)
    assert valid is None and nulls == 0
    assert_same(got, want, f"{op} without bitmaps")


@pytest.mark.parametrize("op", ("ADD", "LESS", "FLOOR_DIV", "TRUE_DIV", "POW", "NULL_MAX", "NULL_EQUALS", "NULL_LOGICAL_OR"))
def test_scalars_on_either_side_valid_and_invalid(gx, T, op):
    """a scalar as lhs and as rhs, valid and invalid (None), beside a nullable column, for every operator family"""
    _, Column, ops = gx
    rng = np.random.default_rng(53)
    n = T + 77
    a = values(rng, "int32", n, True)
    a[a == 0] = 3
    av = rng.random(n) < 0.8
    col = Column.from_numpy(a, av)
    out = np.dtype(np.bool_) if op in ("LESS", "NULL_EQUALS", "NULL_LOGICAL_OR") else np.dtype(np.float64 if op in ("TRUE_DIV", "POW") else np.int32)
    every, none = np.ones(n, bool), np.zeros(n, bool)
    for s in (7, -2, None):
        sv = np.full(n, 7 if s is None else s, dtype=np.int32)
        s_valid = none if s is None else every
        for col_is_lhs in (True, False):
            x, y, lv, rv = (a, sv, av, s_valid) if col_is_lhs else (sv, a, s_valid, av)
            got = ops.binary_operation(col, s, op, out) if col_is_lhs else ops.binary_operation(s, col, op, out)
            want_valid = truth_valid(op, lv, rv, x != 0, y != 0)
            if op in NULL_OPS:
                want = null_op_values(op, x, y, lv, rv, out)
            elif op == "POW":
                with np.errstate(all="ignore"):
                    want = np.power(x.astype(np.float64), y.astype(np.float64))
            else:
                want = expected(op, x, y, out)
            if op == "POW":                  # exponents 0, 1, 2 are exact; the others within the bound of test_pow_accuracy
                assert got.null_count == int((~want_valid).sum())
                g = got.to_numpy()
                assert_same(g, want, f"POW scalar {s}", want_valid & (y >= 0) & (y <= 2))
                ok = want_valid & np.isfinite(want) & (want != 0)
                assert np.array_equal(np.signbit(g[ok]), np.signbit(want[ok]))
                if ok.any():                 # none with the invalid scalar
                    assert int(ulp_distance(np.abs(g[ok]), np.abs(want[ok])).max()) <= 2 * POW_MEASURED_ULP["float64"]
            else:
                check_column(got, want, want_valid, f"{op} scalar {s} col_is_lhs={col_is_lhs}")
    # the scalar's dtype: derived by NumPy's rule beside the column, or given
    got = ops.binary_operation(Column.from_numpy(np.array([1, 2], np.int32)), 0.5, "ADD", np.float64)
    assert got.to_numpy().tolist() == [1.5, 2.5]
    got = ops.binary_operation(Column.from_numpy(np.array([1, 2], np.uint32)), -1, "LESS", np.bool_, scalar_dtype=np.int32)
    assert got.to_numpy().tolist() == [True, True]           # int32(-1) beside uint32: compared as uint32
    got = ops.binary_operation(Column.from_numpy(np.array([1, 2], np.uint32)), -1, "LESS", np.bool_, scalar_dtype=np.int64)
    assert got.to_numpy().tolist() == [False, False]


# ------------------------------------------------------------------------------------------------ unary and cast
@pytest.mark.parametrize("dt", DTYPES)
def test_unary_operators_on_every_dtype_they_support(gx, ROWS, dt):
    cudf_amd, Column, ops = gx
    L = cudf_amd._lib
    rng = np.random.default_rng(59)
    kind = np.dtype(dt).kind
    for n in ROWS:
        if kind == "f":
            a, _ = float_inputs(rng, dt, n)
            halves = (np.arange(n) - n // 2).astype(dt) + np.dtype(dt).type(0.5)
        else:
            a = values(rng, dt, n)
        valid = rng.random(n) < 0.8
        col = Column.from_numpy(a, valid)
        with np.errstate(all="ignore"):
            if kind != "b":
                got = ops.unary_operation(col, "ABS")
                assert got.dtype == np.dtype(dt) and got.null_count == col.null_count and np.array_equal(got.valid_numpy(), valid)
                assert_same(got.to_numpy(), np.abs(a), f"ABS {dt}")
                assert_same(ops.unary_operation(col, "NEGATE").to_numpy(), (-a if kind != "u" else (0 - a).astype(dt)), f"NEGATE {dt}")
            if kind in "iu":
                assert_same(ops.unary_operation(col, "BIT_INVERT").to_numpy(), ~a, f"BIT_INVERT {dt}")
            got = ops.unary_operation(col, "NOT")
            assert got.dtype == np.bool_
            assert_same(got.to_numpy(), a == 0, f"NOT {dt}")
            if kind == "f":
                for v in (a, halves):
                    c = Column.from_numpy(v)
                    assert_same(ops.unary_operation(c, "CEIL").to_numpy(), np.ceil(v), f"CEIL {dt}")
                    assert_same(ops.unary_operation(c, "FLOOR").to_numpy(), np.floor(v), f"FLOOR {dt}")
                    assert_same(ops.unary_operation(c, "RINT").to_numpy(), np.rint(v), f"RINT {dt}")      # halves go to even
                assert_same(ops.is_nan(col).to_numpy(), np.isnan(a), f"IS_NAN {dt}")
                assert_same(ops.is_not_nan(col).to_numpy(), ~np.isnan(a), f"IS_NOT_NAN {dt}")
    for op in L.UNOP:
        code = L.UNOP[op]
        out = L.BOOL8 if op in ("NOT", "IS_NAN", "IS_NOT_NAN") else Column.from_numpy(np.zeros(1, dt)).gx
        if not L.lib.gx_unary_op_supported(code, Column.from_numpy(np.zeros(1, dt)).gx, out):
            with pytest.raises(TypeError):
                ops.unary_operation(Column.from_numpy(np.zeros(3, dt)), op)


def test_abs_negate_extremes_rint_halves_and_nan_payloads(gx):
    _, Column, ops = gx
    for dt in ("int8", "int16", "int32", "int64"):
        info = np.iinfo(dt)
        a = np.array([info.min, info.min + 1, -1, 0, 1, info.max], dtype=dt)
        assert ops.unary_operation(Column.from_numpy(a), "ABS").to_numpy().tolist() == [info.min, info.max, 1, 0, 1, info.max]
        assert ops.unary_operation(Column.from_numpy(a), "NEGATE").to_numpy().tolist() == [info.min, info.max, 1, 0, -1, -info.max]
    u = np.array([0, 1, 255], np.uint8)
    assert ops.unary_operation(Column.from_numpy(u), "ABS").to_numpy().tolist() == [0, 1, 255]
    assert ops.unary_operation(Column.from_numpy(u), "NEGATE").to_numpy().tolist() == [0, 255, 1]
    h = np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 2**52 + 0.0, 0.49999999999999994], np.float64)
    got = ops.unary_operation(Column.from_numpy(h), "RINT").to_numpy()
    assert_same(got, np.array([0.0, 2.0, 2.0, -0.0, -2.0, -2.0, 2**52 + 0.0, 0.0]), "RINT")
    for dt, u, quiet, payloads in (("float64", np.uint64, 0x7FF8 << 48, (1, 0xDEADBEEF, (1 << 51) - 1)), ("float32", np.uint32, 0x7FC0 << 16, (1, 0xBEEF, (1 << 22) - 1))):
        raw = [quiet | p for p in payloads] + [(quiet | payloads[0]) | (1 << (np.dtype(u).itemsize * 8 - 1))]
        raw += [(0x7FF0 << 48 | 5) if dt == "float64" else (0x7F80 << 16 | 5)]                   # a signalling NaN
        a = np.concatenate([np.array(raw, dtype=u).view(dt), np.array([np.inf, -np.inf, 0.0, 1.0], dtype=dt)])
        assert ops.is_nan(Column.from_numpy(a)).to_numpy().tolist() == [True] * 5 + [False] * 4
        assert ops.is_not_nan(Column.from_numpy(a)).to_numpy().tolist() == [False] * 5 + [True] * 4


def test_is_null_is_valid_on_a_sliced_nullable_column(gx, T):
    """gx_bitmask_to_bool8 from begin bits 0 / 1 / 31 / 33 (a sliced view) and through ops.is_null / is_valid"""
    import torch
    cudf_amd, Column, ops = gx
    L = cudf_amd._lib
    from cudf_amd.column import ptr, stream_ptr, pack_mask
    rng = np.random.default_rng(61)
    for n in (1, 15, 16, 17, 33, T - 1, T + 1, 3 * T + 17):
        for bit in BEGIN_BITS:
            buf = rng.random(bit + n + 9) < 0.7
            words = torch.from_numpy(pack_mask(buf).view(np.int32).copy()).cuda()
            for invert in (0, 1):
                out = torch.full((n + 16,), 7, dtype=torch.uint8, device="cuda")
                assert L.lib.gx_bitmask_to_bool8(ptr(words), bit, n, invert, ptr(out), stream_ptr()) == 0
                h = out.cpu().numpy()
                assert (h[n:] == 7).all()
                assert np.array_equal(h[:n], (buf[bit:bit + n] ^ bool(invert)).astype(np.uint8)), (n, bit, invert)
    a = values(rng, "int32", 1000)
    valid = rng.random(1000) < 0.6
    col = Column.from_numpy(a, valid)
    assert np.array_equal(ops.is_null(col).to_numpy(), ~valid) and ops.is_null(col).mask is None
    assert np.array_equal(ops.is_valid(col).to_numpy(), valid)
    assert np.array_equal(col.isnull().to_numpy(), ~valid) and np.array_equal(col.notnull().to_numpy(), valid)
    plain = Column.from_numpy(a)
    assert not ops.is_null(plain).to_numpy().any() and ops.is_valid(plain).to_numpy().all()


def cast_values(rng, src, dst, n):
    """values of src that are in range of dst where the cast would otherwise be unspecified (float -> integer)"""
    src, dst = np.dtype(src), np.dtype(dst)
    if src.kind == "f" and dst.kind in "iu":
        info = np.iinfo(dst)
        lo, hi = max(info.min, -2**23), min(info.max, 2**23)
        v = rng.integers(lo, hi, n, endpoint=True).astype(src)
        frac = rng.integers(0, 4, n).astype(src) / src.type(4)
        return np.where((v + frac <= hi) & (v - frac >= lo), v + np.where(v < 0, -frac, frac), v).astype(src)
    if src.kind == "f":
        v, _ = float_inputs(rng, src, n)
        return v
    return values(rng, src, n)


@pytest.mark.parametrize("src", DTYPES)
def test_cast_every_pair(gx, T, src):
    """static_cast from src to each of the 11 dtypes: a negative value to unsigned wraps, float to integer truncates toward zero,
    anything to BOOL8 is x != 0; validity and null count are the input's"""
    _, Column, ops = gx
    rng = np.random.default_rng(67)
    n = T + 19
    for dst in DTYPES:
        a = cast_values(rng, src, dst, n)
        valid = rng.random(n) < 0.8
        got = ops.cast(Column.from_numpy(a, valid), dst)
        assert got.dtype == np.dtype(dst) and got.null_count == int((~valid).sum()) and np.array_equal(got.valid_numpy(), valid)
        assert_same(got.to_numpy(), cast(a, dst), f"cast {src} -> {dst}")
        assert_same(Column.from_numpy(a).astype(dst).to_numpy(), cast(a, dst), f"astype {src} -> {dst}")
    if np.dtype(src).kind == "f":
        a = np.array([1.9, -1.9, 0.99, -0.99, 127.9, -128.9, 2.5, -2.5], dtype=src)
        assert ops.cast(Column.from_numpy(a), np.int8).to_numpy().tolist() == [1, -1, 0, 0, 127, -128, 2, -2]
    if np.dtype(src).kind == "i":
        a = np.array([-1, -2, 0, 1], dtype=src)
        assert ops.cast(Column.from_numpy(a), np.uint64).to_numpy().tolist() == [2**64 - 1, 2**64 - 2, 0, 1]


# ------------------------------------------------------------------------------------------------ Column operators, DataFrame
def test_column_operators_against_numpy(gx):
    """each dunder once against NumPy with NumPy's promotion, the two pairs where the operands are cast first among them"""
    import operator as o
    _, Column, ops = gx
    rng = np.random.default_rng(71)
    n = 1500
    pairs = [("int32", "int32"), ("int32", "uint32"), ("int64", "uint64"), ("int8", "float32"), ("int64", "float32"), ("uint8", "int8"),
             ("float32", "float64"), ("bool", "int16")]
    for ld, rd in pairs:
        a, b = values(rng, ld, n, True), values(rng, rd, n, True)
        b = safe_divisor(a, b)
        ca, cb = Column.from_numpy(a), Column.from_numpy(b)
        for f in (o.add, o.sub, o.mul, o.truediv, o.floordiv, o.mod, o.lt, o.le, o.gt, o.ge):
            if f is o.sub and "bool" in (ld, rd) and ld == rd:
                continue
            with np.errstate(all="ignore"):
                want = f(a, b)
            got = f(ca, cb)
            assert got.dtype == want.dtype, (f.__name__, ld, rd, got.dtype, want.dtype)
            assert_same(got.to_numpy(), want, f"{f.__name__} {ld} {rd}")
        assert_same(ca.eq(cb).to_numpy(), a == b, "eq")
        assert_same(ca.ne(cb).to_numpy(), a != b, "ne")
    # the full-range pairs where NumPy promotes beyond the common type of C++: the operands are cast first
    a, b = values(rng, "int32", n), values(rng, "uint32", n)
    got = Column.from_numpy(a) + Column.from_numpy(b)
    assert got.dtype == np.int64
    assert_same(got.to_numpy(), a + b, "int32 + uint32")
    assert_same((Column.from_numpy(a) < Column.from_numpy(b)).to_numpy(), a < b, "int32 < uint32")
    a, b = values(rng, "int64", n), values(rng, "uint64", n)
    got = Column.from_numpy(a) + Column.from_numpy(b)
    assert got.dtype == np.float64
    assert_same(got.to_numpy(), a + b, "int64 + uint64")
    # integers only
    a, b = values(rng, "int32", n), rng.integers(0, 31, n).astype(np.int32)
    ca, cb = Column.from_numpy(a), Column.from_numpy(b)
    for f in (o.and_, o.or_, o.xor, o.lshift, o.rshift):
        assert_same(f(ca, cb).to_numpy(), f(a, b), f.__name__)
    e = rng.integers(0, 6, n).astype(np.int32)
    assert_same((ca ** Column.from_numpy(e)).to_numpy(), a ** e, "int pow")
    x, y = (100.0 * (1.0 - rng.random(n))), rng.integers(-2, 3, n).astype(np.float64)
    got = (Column.from_numpy(x) ** Column.from_numpy(y)).to_numpy()
    assert np.allclose(got, x ** y, rtol=1e-14, atol=0)
    assert_same((~ca).to_numpy(), ~a, "invert")
    assert_same((-ca).to_numpy(), -a, "neg")
    assert_same(abs(ca).to_numpy(), np.abs(a), "abs")
    p, q = rng.integers(0, 2, n).astype(bool), rng.integers(0, 2, n).astype(bool)
    cp, cq = Column.from_numpy(p), Column.from_numpy(q)
    for f in (o.and_, o.or_, o.xor):
        got = f(cp, cq)
        assert got.dtype == np.bool_
        assert_same(got.to_numpy(), f(p, q), f.__name__)
    assert_same((~cp).to_numpy(), ~p, "invert bool")


def test_reflected_operators_with_python_scalars(gx):
    import operator as o
    _, Column, ops = gx
    rng = np.random.default_rng(73)
    n = 700
    for dt in ("int32", "float32", "uint8", "float64"):
        a = values(rng, dt, n, True)
        a[a == 0] = 2
        c = Column.from_numpy(a)
        for s in (3, 2.5):
            for f in (o.add, o.sub, o.mul, o.truediv, o.floordiv, o.mod):
                with np.errstate(all="ignore"):
                    w1, w2 = f(a, s), f(s, a)
                g1, g2 = f(c, s), f(s, c)
                assert g1.dtype == w1.dtype and g2.dtype == w2.dtype, (f.__name__, dt, s)
                assert_same(g1.to_numpy(), w1, f"{f.__name__} {dt} {s}")
                assert_same(g2.to_numpy(), w2, f"r{f.__name__} {dt} {s}")
            assert_same((c < s).to_numpy(), a < s, "lt")
            assert_same((c > s).to_numpy(), a > s, "gt")
            assert_same((s < c).to_numpy(), s < a, "reflected lt")
            assert_same(c.eq(s).to_numpy(), a == s, "eq")
            assert_same(c.ne(s).to_numpy(), a != s, "ne")
    a = values(rng, "int32", n)
    c = Column.from_numpy(a)
    assert_same((5 & c).to_numpy(), 5 & a, "rand")
    assert_same((5 | c).to_numpy(), 5 | a, "ror")
    assert_same((5 ^ c).to_numpy(), 5 ^ a, "rxor")
    s = Column.from_numpy(rng.integers(0, 20, n).astype(np.int32))
    assert_same((3 << s).to_numpy(), 3 << s.to_numpy(), "rlshift")
    assert_same((-1000 >> s).to_numpy(), -1000 >> s.to_numpy(), "rrshift")
    assert_same((2 ** s).to_numpy(), 2 ** s.to_numpy(), "rpow")
    assert_same((c ** 2).to_numpy(), a ** 2, "pow")
    # identity comparison and hashing are untouched
    assert (c == c) is True and (c == Column.from_numpy(a)) is False and len({c, c}) == 1


def test_dataframe_expressions_against_pandas(gx):
    import pandas as pd
    cudf_amd, Column, ops = gx
    rng = np.random.default_rng(79)
    n = 20_011
    pdf = pd.DataFrame({"a": rng.integers(-1000, 1000, n).astype(np.int64), "b": rng.integers(-1000, 1000, n).astype(np.int32),
                        "x": rng.standard_normal(n)})
    df = cudf_amd.DataFrame.from_pandas(pdf)
    df["c"] = df["a"] * df["b"] + 1
    pdf["c"] = pdf["a"] * pdf["b"] + 1
    df["y"] = df["x"] * 2.0 - df["a"] / 3
    pdf["y"] = pdf["x"] * 2.0 - pdf["a"] / 3
    pd.testing.assert_frame_equal(df.to_pandas(), pdf, check_exact=True)
    got = df[(df["a"] > df["b"]) & (df["b"] > 0)].to_pandas()
    want = pdf[(pdf["a"] > pdf["b"]) & (pdf["b"] > 0)].reset_index(drop=True)
    pd.testing.assert_frame_equal(got, want, check_exact=True)
    assert len(want) > 0


# ------------------------------------------------------------------------------------------------ the C++ surface
def test_cpp_surface_cases():
    """cudf::binary_operation (three overloads), unary_operation, cast, is_null / is_valid / is_nan on views made by cudf::slice"""
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "cudf_binaryop_tests")], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:])
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "18 run, 0 failed" in r.stdout
