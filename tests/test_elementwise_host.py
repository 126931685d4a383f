"""CPU: cudf::binary_operation / unary_operation / cast as far as they can be checked without a device -- exported symbols, the
argument checks of gx_binary_op / gx_unary_op / gx_cast / gx_bitmask_to_bool8 (NULL pointers: nothing is launched), the
_supported tables, the --host cases of the C++ surface, the argument checks of the Python surface, and a NumPy model of the
validity rules of gx_elementwise.hip (out_bits: AND-composition of two bitmaps read at independent begin bits, the six NULL_*
operators), checked exhaustively over all 4 x 4 (validity, truth) pairs and the begin bits 0 / 1 / 31 / 33.  The same model is the
reference of tests/test_gpu_elementwise.py."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "cudf_amd", "libcudf.so")
BIN = os.path.join(ROOT, "tests", "cpp", "cudf_binaryop_tests")

GX_EINVAL, GX_EDTYPE = -1, -2
DTYPES = range(1, 12)
FLOATS = (9, 10)
BOOL8 = 11
NEW = ("gx_binary_op", "gx_unary_op", "gx_cast", "gx_bitmask_to_bool8", "gx_binary_op_supported", "gx_unary_op_supported",
       "gx_elementwise_tile_rows", "gx_elementwise_grid_cap")


def _build():
    import __graft_entry__ as ge
    ge.build()


@pytest.fixture(autouse=True, scope="module")
def _the_kernel_layer_has_the_operators():
    _build()
    from cudf_amd import _lib
    assert hasattr(_lib.lib, "gx_binary_op") and "gx_binary_op" in _lib.EXPORTED


def test_libraries_export_the_elementwise_api():
    syms = subprocess.check_output(["nm", "-DC", "--defined-only", LIB], text=True)
    for s, overloads in (("cudf::binary_operation(", 3), ("cudf::unary_operation(", 1), ("cudf::cast(", 1), ("cudf::is_null(", 1),
                         ("cudf::is_valid(", 1), ("cudf::is_nan(", 1), ("cudf::is_not_nan(", 1), ("cudf::is_supported_cast(", 1)):
        assert syms.count(s) == overloads, f"libcudf.so exports {syms.count(s)} overloads of {s}"
    und = subprocess.check_output(["nm", "-D", "--undefined-only", LIB], text=True)
    from cudf_amd import _lib
    for s in ("gx_binary_op", "gx_unary_op", "gx_cast", "gx_bitmask_to_bool8"):
        assert s in und
    for s in NEW:
        assert s in _lib.EXPORTED and hasattr(_lib.lib, s)
    for h in ("binaryop.hpp", "unary.hpp"):
        assert os.path.exists(os.path.join(ROOT, "include", "cudf", h))


def test_operator_codes_mirror_the_header():
    """gx_binop / gx_unop in gx.h, L.BINOP / L.UNOP in the binding: one list"""
    import re
    from cudf_amd import _lib as L
    text = open(os.path.join(ROOT, "include", "cudf_amd", "gx.h")).read()
    b = {m.group(1): int(m.group(2)) for m in re.finditer(r"GX_BINOP_([A-Z0-9_]+) = (\d+)", text)}
    u = {m.group(1): int(m.group(2)) for m in re.finditer(r"GX_UNOP_([A-Z0-9_]+) = (\d+)", text)}
    assert b == L.BINOP and len(b) == 34
    assert u == L.UNOP and len(u) == 26


def test_tile_rows_and_grid_cap():
    from cudf_amd import _lib as L
    T = L.lib.gx_elementwise_tile_rows()
    assert T > 0 and T % 32 == 0          # a tile owns whole validity words: one writer per word
    assert L.lib.gx_elementwise_grid_cap() > 0


def _binop(lib, op=0, ld=4, lhs=0x10000, lbit=0, lscalar=0, rd=4, rhs=0x20000, rbit=0, rscalar=0, n=7, od=4, out=0x30000, out_valid=None):
    p = lambda x: ctypes.c_void_p(x) if x else None  # noqa: E731
    return lib.gx_binary_op(op, ld, p(lhs), None, lbit, None, lscalar, rd, p(rhs), None, rbit, None, rscalar, n, od, p(out), out_valid,
                            None, None)


def test_binary_op_misuse_is_rejected_before_any_device_call():
    from cudf_amd import _lib as L
    lib = L.lib
    for n in (-1, 2**31, 2**40):
        assert _binop(lib, n=n) == GX_EINVAL, n
    assert _binop(lib, lbit=-1) == GX_EINVAL and _binop(lib, rbit=-1) == GX_EINVAL
    assert _binop(lib, lhs=None) == GX_EINVAL and _binop(lib, rhs=None) == GX_EINVAL and _binop(lib, out=None) == GX_EINVAL
    for op in (-1, 34, 1000):
        assert _binop(lib, op=op) == GX_EINVAL, op
    for d in (0, 12, 99, -3):
        assert _binop(lib, ld=d) == GX_EDTYPE and _binop(lib, rd=d) == GX_EDTYPE and _binop(lib, od=d) == GX_EDTYPE, d
    for op in ("LOG_BASE", "ATAN2", "GENERIC_BINARY"):
        assert _binop(lib, op=L.BINOP[op]) == GX_EDTYPE, op
    assert _binop(lib, op=L.BINOP["BITWISE_AND"], ld=L.FLOAT64) == GX_EDTYPE
    assert _binop(lib, op=L.BINOP["INT_POW"], rd=L.FLOAT32) == GX_EDTYPE
    # no rows: 0, whatever the pointers -- for every operator that is built and every dtype
    for op in range(34):
        for d in DTYPES:
            if lib.gx_binary_op_supported(op, d, d, d):
                for ls, rs in itertools.product((0, 1), repeat=2):
                    assert _binop(lib, op=op, ld=d, rd=d, od=d, n=0, lhs=None, rhs=None, out=None, lscalar=ls, rscalar=rs) == 0


def test_unary_cast_and_bitmask_misuse_is_rejected_before_any_device_call():
    from cudf_amd import _lib as L
    lib = L.lib
    a, o = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000)
    ABS, SQRT, NOT = L.UNOP["ABS"], L.UNOP["SQRT"], L.UNOP["NOT"]
    for n in (-1, 2**31, 2**40):
        assert lib.gx_unary_op(ABS, L.INT32, a, n, L.INT32, o, None) == GX_EINVAL
        assert lib.gx_cast(L.INT32, a, n, L.INT64, o, None) == GX_EINVAL
        assert lib.gx_bitmask_to_bool8(a, 0, n, 0, o, None) == GX_EINVAL
    assert lib.gx_unary_op(ABS, L.INT32, None, 5, L.INT32, o, None) == GX_EINVAL
    assert lib.gx_unary_op(ABS, L.INT32, a, 5, L.INT32, None, None) == GX_EINVAL
    for op in (-1, 24, 99, 102):
        assert lib.gx_unary_op(op, L.INT32, a, 5, L.INT32, o, None) == GX_EINVAL, op
    for d in (0, 12, -1):
        assert lib.gx_unary_op(ABS, d, a, 5, L.INT32, o, None) == GX_EDTYPE
        assert lib.gx_unary_op(NOT, L.INT32, a, 5, d, o, None) == GX_EDTYPE
        assert lib.gx_cast(d, a, 5, L.INT32, o, None) == GX_EDTYPE and lib.gx_cast(L.INT32, a, 5, d, o, None) == GX_EDTYPE
    assert lib.gx_unary_op(SQRT, L.INT32, a, 5, L.INT32, o, None) == GX_EDTYPE          # a float operator on an integer
    assert lib.gx_unary_op(ABS, L.INT32, a, 5, L.INT64, o, None) == GX_EDTYPE           # out_dtype != in_dtype
    assert lib.gx_unary_op(L.UNOP["SIN"], L.FLOAT64, a, 5, L.FLOAT64, o, None) == GX_EDTYPE
    assert lib.gx_cast(L.INT32, None, 5, L.INT64, o, None) == GX_EINVAL and lib.gx_cast(L.INT32, a, 5, L.INT64, None, None) == GX_EINVAL
    assert lib.gx_bitmask_to_bool8(a, -1, 5, 0, o, None) == GX_EINVAL and lib.gx_bitmask_to_bool8(a, 0, 5, 0, None, None) == GX_EINVAL
    for d in DTYPES:
        assert lib.gx_unary_op(NOT, d, None, 0, L.BOOL8, None, None) == 0
        for d2 in DTYPES:
            assert lib.gx_cast(d, None, 0, d2, None, None) == 0
    assert lib.gx_bitmask_to_bool8(None, 0, 0, 1, None, None) == 0


def test_supported_tables():
    from cudf_amd import _lib as L
    lib = L.lib
    integer_only = {"BITWISE_AND", "BITWISE_OR", "BITWISE_XOR", "SHIFT_LEFT", "SHIFT_RIGHT", "SHIFT_RIGHT_UNSIGNED", "INT_POW"}
    unbuilt = {"LOG_BASE", "ATAN2", "GENERIC_BINARY"}
    for name, op in L.BINOP.items():
        for l, r, o in itertools.product(DTYPES, repeat=3):
            want = name not in unbuilt and not (name in integer_only and (l in FLOATS or r in FLOATS))
            assert lib.gx_binary_op_supported(op, l, r, o) == int(want), (name, l, r, o)
        assert lib.gx_binary_op_supported(op, 0, 4, 4) == 0 and lib.gx_binary_op_supported(op, 4, 12, 4) == 0
        assert lib.gx_binary_op_supported(op, 4, 4, 99) == 0
    assert lib.gx_binary_op_supported(34, 4, 4, 4) == 0 and lib.gx_binary_op_supported(-1, 4, 4, 4) == 0
    same = {"ABS": lambda d: d != BOOL8, "NEGATE": lambda d: d != BOOL8, "SQRT": lambda d: d in FLOATS, "CEIL": lambda d: d in FLOATS,
            "FLOOR": lambda d: d in FLOATS, "RINT": lambda d: d in FLOATS, "BIT_INVERT": lambda d: d not in FLOATS and d != BOOL8}
    to_bool = {"NOT": lambda d: True, "IS_NAN": lambda d: d in FLOATS, "IS_NOT_NAN": lambda d: d in FLOATS}
    for name, op in L.UNOP.items():
        for i, o in itertools.product(DTYPES, repeat=2):
            if name in same:
                want = same[name](i) and o == i
            elif name in to_bool:
                want = to_bool[name](i) and o == BOOL8
            else:
                want = False                 # the transcendental operators, CBRT, BIT_COUNT
            assert lib.gx_unary_op_supported(op, i, o) == int(want), (name, i, o)


def test_cpp_host_cases_run_without_a_device():
    """every throw of the C++ surface, the empty results and the enumerators' values: decided before the first device call"""
    _build()
    r = subprocess.run([BIN, "--host"], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "6 run, 0 failed" in r.stdout
    assert "[ OK ] binary_operation: a size mismatch throws cudf::logic_error \"Column sizes don't match\"" in r.stdout
    assert "[ OK ] binary_operation: operators that are not built throw cudf::logic_error" in r.stdout


def test_public_headers_compile_clean(tmp_path):
    """gx.h as C99 -pedantic, binaryop.hpp and unary.hpp alone (each includes what it needs) as C++20 -Wall -Wextra -Werror"""
    inc = ["-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include"]
    c = tmp_path / "abi.c"
    c.write_text("#include <cudf_amd/gx.h>\nint main(void) { return GX_BINOP_NULL_LOGICAL_OR == 33 && GX_UNOP_NEGATE == 23 ? 0 : 1; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", *inc, str(c)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for h in ("cudf/binaryop.hpp", "cudf/unary.hpp"):
        cpp = tmp_path / "api.cpp"
        cpp.write_text(f"#include <{h}>\nint main() {{ return 0; }}\n")
        r = subprocess.run(["g++", "-std=c++20", "-Wall", "-Wextra", "-Werror", "-D__HIP_PLATFORM_AMD__", "-fsyntax-only", *inc, str(cpp)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]


def test_python_surface_rejects_bad_arguments_without_a_device():
    from cudf_amd import Column, ops
    i64, i32, f64, b = (lambda n, dt=dt: Column(None, dt, n) for dt in (np.int64, np.int32, np.float64, np.bool_))
    with pytest.raises(ValueError):
        ops.binary_operation(i64(3), i64(4), "ADD", np.int64)
    with pytest.raises(ValueError):
        ops.binary_operation(i64(3), i64(3), "PLUS", np.int64)
    with pytest.raises(TypeError):
        ops.binary_operation(1, 2, "ADD", np.int64)
    with pytest.raises(TypeError):
        ops.binary_operation(i64(3), f64(3), "BITWISE_AND", np.int64)
    with pytest.raises(TypeError):
        ops.binary_operation(i64(3), i64(3), "ATAN2", np.float64)
    with pytest.raises(TypeError):
        ops.binary_operation(i64(3), i64(3), "ADD", np.complex64)
    with pytest.raises(TypeError):
        ops.unary_operation(i32(3), "SQRT")
    with pytest.raises(TypeError):
        ops.unary_operation(f64(3), "SIN")
    with pytest.raises(ValueError):
        ops.unary_operation(f64(3), "SQUARE")
    with pytest.raises(TypeError):
        ops.is_nan(i32(3))
    with pytest.raises(TypeError):
        ops.cast(i32(3), np.complex128)
    with pytest.raises(TypeError):
        f64(3) & f64(3)
    with pytest.raises(TypeError):
        i32(3) << 1.5
    with pytest.raises(TypeError):
        i32(3) + "x"
    # columns are still compared and hashed by identity
    c = i64(3)
    assert (c == c) is True and (c != i64(3)) is True and len({c, c, i64(3)}) == 2


# ------------------------------------------------------------------------------------------------ the model of the validity rules
# One output word of 32 rows from two bitmaps read at independent begin bits, as the kernel composes it: every thread takes the
# R bits of its rows from each operand (bits_from of gx_validity.hpp: two words only when the run crosses a word), out_bits applies the operator's
# rule, the lanes that share the word OR their pieces together.

def bits_from(words, sb, cnt, reads=None):
    w, sh = sb >> 5, sb & 31
    two = int(words[w])
    if reads is not None:
        reads.append(w)
    if sh + cnt > 32:
        two |= int(words[w + 1]) << 32
        if reads is not None:
            reads.append(w + 1)
    v = (two >> sh) & 0xFFFFFFFF
    return v if cnt == 32 else v & ((1 << cnt) - 1)


def pack(bits):
    pad = np.zeros((len(bits) + 31) // 32 * 32, dtype=np.uint8)
    pad[:len(bits)] = bits
    return np.packbits(pad, bitorder="little").view(np.uint32)


def out_bits(op, lb, rb, tx, ty, lm):
    """lb / rb: validity bits, tx / ty: truth bits (value != 0) of the rows of one thread; lm: the rows that exist"""
    if op in ("NULL_EQUALS", "NULL_NOT_EQUALS"):
        return lm
    if op in ("NULL_MAX", "NULL_MIN"):
        return (lb | rb) & lm
    if op == "NULL_LOGICAL_AND":
        return ((lb & rb) | (lb & ~tx) | (rb & ~ty)) & lm
    if op == "NULL_LOGICAL_OR":
        return ((lb & rb) | (lb & tx) | (rb & ty)) & lm
    return lb & rb & lm


def model_valid_words(op, lwords, lbit, rwords, rbit, xt, yt, n, R):
    """the (n + 31) / 32 output words; lwords / rwords None = no bitmap (all valid)"""
    words = []
    for w0 in range(0, n, 32):
        word = 0
        for row0 in range(w0, min(w0 + 32, n), R):
            cnt = min(R, n - row0)
            lm = (1 << cnt) - 1
            reads = []
            lb = bits_from(lwords, lbit + row0, cnt, reads) if lwords is not None else lm
            if lwords is not None:
                assert max(reads) <= (lbit + n - 1) >> 5         # no word behind the operand's last bit is read
            rb = bits_from(rwords, rbit + row0, cnt) if rwords is not None else lm
            tx = sum(int(bool(xt[row0 + k])) << k for k in range(cnt))
            ty = sum(int(bool(yt[row0 + k])) << k for k in range(cnt))
            word |= out_bits(op, lb, rb, tx, ty, lm) << (row0 - w0)
        words.append(word)
    return words


def truth_valid(op, lv, rv, xt, yt):
    """the rule of the issue, row by row, in plain NumPy"""
    if op in ("NULL_EQUALS", "NULL_NOT_EQUALS"):
        return np.ones(len(lv), dtype=bool)
    if op in ("NULL_MAX", "NULL_MIN"):
        return lv | rv
    if op == "NULL_LOGICAL_AND":
        return (lv & rv) | (lv & ~xt) | (rv & ~yt)
    if op == "NULL_LOGICAL_OR":
        return (lv & rv) | (lv & xt) | (rv & yt)
    return lv & rv


OPS = ("ADD", "NULL_EQUALS", "NULL_NOT_EQUALS", "NULL_MAX", "NULL_MIN", "NULL_LOGICAL_AND", "NULL_LOGICAL_OR")
BEGIN_BITS = (0, 1, 31, 33)


def test_model_of_the_validity_rules_all_pairs_and_begin_bits():
    """all 4 x 4 (validity, truth) pairs of one row, laid out so that every pair sits at every position of a thread's run, for every
    R the kernels use, with the operands' bitmaps at independent begin bits and noise around them"""
    rng = np.random.default_rng(7)
    states = list(itertools.product((0, 1), repeat=4))        # (lv, xt, rv, yt): 16 combinations
    base = np.array(states * 5 + [states[i] for i in rng.permutation(16)], dtype=bool)     # 96 rows
    cases = 0
    for op in OPS:
        for R in (2, 4, 8, 16):
            for n in (len(base), len(base) - 1, 33, 17):
                rows = base[:n]
                lv, xt, rv, yt = rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]
                for lbit, rbit in itertools.product(BEGIN_BITS, repeat=2):
                    lbuf = rng.integers(0, 2, lbit + n + 2).astype(np.uint8)
                    rbuf = rng.integers(0, 2, rbit + n + 2).astype(np.uint8)
                    lbuf[lbit:lbit + n] = lv
                    rbuf[rbit:rbit + n] = rv
                    got = model_valid_words(op, pack(lbuf), lbit, pack(rbuf), rbit, xt, yt, n, R)
                    want = pack(truth_valid(op, lv, rv, xt, yt).astype(np.uint8))
                    assert [int(w) for w in want[:len(got)]] == got, (op, R, n, lbit, rbit)
                    cases += 1
    assert cases == len(OPS) * 4 * 4 * 16


def test_model_kleene_truth_tables():
    """the 16 (validity, truth) pairs of NULL_LOGICAL_AND / OR written out: the value a valid row must carry"""
    T, F, N = (1, 1), (1, 0), (0, 0)         # (valid, truth); a null's truth is arbitrary: both are tried
    and_table = {(T, T): 1, (T, F): 0, (F, T): 0, (F, F): 0, (T, N): None, (N, T): None, (F, N): 0, (N, F): 0, (N, N): None}
    or_table = {(T, T): 1, (T, F): 1, (F, T): 1, (F, F): 0, (T, N): 1, (N, T): 1, (F, N): None, (N, F): None, (N, N): None}
    for table, op in ((and_table, "NULL_LOGICAL_AND"), (or_table, "NULL_LOGICAL_OR")):
        for (l, r), want in table.items():
            for lt, rt in itertools.product((0, 1), repeat=2):
                lv, xt = l[0], (l[1] if l[0] else lt)
                rv, yt = r[0], (r[1] if r[0] else rt)
                ob = out_bits(op, lv, rv, xt, yt, 1)
                assert ob == (want is not None), (op, l, r)
                if want is not None:             # the kernel's value formula (apply_rows)
                    val = ((not lv or xt) and (not rv or yt)) if op == "NULL_LOGICAL_AND" else ((lv and xt) or (rv and yt))
                    assert int(bool(val)) == want, (op, l, r)
