"""A NumPy model of cudf_amd's expression evaluator, shared by tests/test_expression_host.py and tests/test_gpu_expression.py:
the type rules of include/cudf_amd/gx.h written out as a table, the value and validity of every built operator, a recursive
evaluation of a node array, an interpreter of the accumulator machine that gx_expr_plan describes, and a seeded generator of
random node arrays.  Nothing here touches a device.  Where the contract leaves a value unspecified (integer division by zero, a
cast out of range, the data of a null row) the model picks something deterministic: both evaluations run the same functions, so
they still have to agree bit for bit."""
import numpy as np

INT8, INT16, INT32, INT64, UINT8, UINT16, UINT32, UINT64, FLOAT32, FLOAT64, BOOL8 = range(1, 12)
DTYPES = tuple(range(1, 12))
NP = {INT8: np.int8, INT16: np.int16, INT32: np.int32, INT64: np.int64, UINT8: np.uint8, UINT16: np.uint16, UINT32: np.uint32,
      UINT64: np.uint64, FLOAT32: np.float32, FLOAT64: np.float64, BOOL8: np.bool_}
GX = {np.dtype(v): k for k, v in NP.items()}
FLOATS = (FLOAT32, FLOAT64)

AST_OPS = ("ADD", "SUB", "MUL", "DIV", "TRUE_DIV", "FLOOR_DIV", "MOD", "PYMOD", "POW", "EQUAL", "NULL_EQUAL", "NOT_EQUAL", "LESS",
           "GREATER", "LESS_EQUAL", "GREATER_EQUAL", "BITWISE_AND", "BITWISE_OR", "BITWISE_XOR", "LOGICAL_AND", "NULL_LOGICAL_AND",
           "LOGICAL_OR", "NULL_LOGICAL_OR", "IDENTITY", "IS_NULL", "SIN", "COS", "TAN", "ARCSIN", "ARCCOS", "ARCTAN", "SINH", "COSH",
           "TANH", "ARCSINH", "ARCCOSH", "ARCTANH", "EXP", "LOG", "SQRT", "CBRT", "CEIL", "FLOOR", "ABS", "RINT", "BIT_INVERT", "NOT",
           "CAST_TO_INT64", "CAST_TO_UINT64", "CAST_TO_FLOAT64")
OP = {name: i for i, name in enumerate(AST_OPS)}
FIRST_UNARY = OP["IDENTITY"]
BINARY_OPS = AST_OPS[:FIRST_UNARY]
UNARY_OPS = AST_OPS[FIRST_UNARY:]
NOT_BUILT = ("SIN", "COS", "TAN", "ARCSIN", "ARCCOS", "ARCTAN", "SINH", "COSH", "TANH", "ARCSINH", "ARCCOSH", "ARCTANH", "EXP", "LOG",
             "CBRT")
COLUMN, LITERAL, UNARY, BINARY = range(4)                       # gx_expr_node_kind
LOAD, APPLY, APPLY_REV, APPLY_UNARY, SPILL = range(5)            # gx_expr_instr_kind
SRC_COLUMN, SRC_LITERAL, SRC_SLOT = range(3)


def cls(t):
    """C(T) as a dtype code: INT32 for BOOL8 and everything narrower than 32 bits"""
    return t if t in (INT32, INT64, UINT32, UINT64, FLOAT32, FLOAT64) else INT32


# ------------------------------------------------------------------------------------------------ the type table, written out
def result_dtype(op, t):
    """the result dtype of operator `op` (a name) on operands of dtype t, or None for a type error"""
    is_float, is_bool = t in FLOATS, t == BOOL8
    if op in ("ADD", "SUB", "MUL", "DIV", "MOD", "PYMOD"):
        return cls(t)
    if op in ("TRUE_DIV", "FLOOR_DIV"):
        return FLOAT64
    if op == "POW":
        return FLOAT32 if t == FLOAT32 else FLOAT64
    if op in ("BITWISE_AND", "BITWISE_OR", "BITWISE_XOR"):
        return None if is_float else cls(t)
    if op in ("EQUAL", "NOT_EQUAL", "LESS", "GREATER", "LESS_EQUAL", "GREATER_EQUAL", "LOGICAL_AND", "LOGICAL_OR", "NULL_EQUAL",
              "NULL_LOGICAL_AND", "NULL_LOGICAL_OR", "IS_NULL", "NOT"):
        return BOOL8
    if op == "IDENTITY":
        return t
    if op == "ABS":
        return None if is_bool else cls(t)
    if op == "BIT_INVERT":
        return None if is_float or is_bool else cls(t)
    if op in ("SQRT", "CEIL", "FLOOR", "RINT"):
        return t if is_float else None
    if op in ("CAST_TO_INT64", "CAST_TO_UINT64", "CAST_TO_FLOAT64"):
        return {"CAST_TO_INT64": INT64, "CAST_TO_UINT64": UINT64, "CAST_TO_FLOAT64": FLOAT64}[op]
    return None                                                  # the transcendental operators and CBRT


# ------------------------------------------------------------------------------------------------ values and validity
def _as_class(a, t):
    return a.astype(NP[cls(t)])


def _nz(b):
    return np.where(b == 0, np.ones((), b.dtype), b)


def binary_value(op, t, a, av, b, bv):
    """(values, validity) of `op` on two operand arrays of dtype t with validity av / bv"""
    x, y = _as_class(a, t), _as_class(b, t)
    both = av & bv
    isf = t in FLOATS
    with np.errstate(all="ignore"):
        if op == "ADD":
            return x + y, both
        if op == "SUB":
            return x - y, both
        if op == "MUL":
            return x * y, both
        if op == "DIV":
            if isf:
                return x / y, both
            r = np.fmod(x, _nz(y))
            return np.where(y == 0, 0, (x - r) // _nz(y)).astype(x.dtype), both
        if op == "MOD":
            return (np.fmod(x, y) if isf else np.where(y == 0, 0, np.fmod(x, _nz(y))).astype(x.dtype)), both
        if op == "PYMOD":
            return (np.remainder(x, y) if isf else np.where(y == 0, 0, np.remainder(x, _nz(y))).astype(x.dtype)), both
        if op == "TRUE_DIV":
            return x.astype(np.float64) / y.astype(np.float64), both
        if op == "FLOOR_DIV":
            return np.floor(x.astype(np.float64) / y.astype(np.float64)), both
        if op == "POW":
            return (np.power(x, y) if t == FLOAT32 else np.power(x.astype(np.float64), y.astype(np.float64))), both
        if op == "BITWISE_AND":
            return x & y, both
        if op == "BITWISE_OR":
            return x | y, both
        if op == "BITWISE_XOR":
            return x ^ y, both
        cmp = {"EQUAL": np.equal, "NOT_EQUAL": np.not_equal, "LESS": np.less, "GREATER": np.greater, "LESS_EQUAL": np.less_equal,
               "GREATER_EQUAL": np.greater_equal}
        if op in cmp:
            return cmp[op](x, y), both
        tx, ty = x != 0, y != 0
        if op == "LOGICAL_AND":
            return tx & ty, both
        if op == "LOGICAL_OR":
            return tx | ty, both
        if op == "NULL_EQUAL":
            return np.where(both, x == y, av == bv), np.ones_like(av)
        if op == "NULL_LOGICAL_AND":
            return (~av | tx) & (~bv | ty), both | (av & ~tx) | (bv & ~ty)
        if op == "NULL_LOGICAL_OR":
            return (av & tx) | (bv & ty), both | (av & tx) | (bv & ty)
    raise AssertionError(op)


def unary_value(op, t, a, av):
    x = _as_class(a, t)
    with np.errstate(all="ignore"):
        if op == "IDENTITY":
            return a, av
        if op == "IS_NULL":
            return ~av, np.ones_like(av)
        if op == "NOT":
            return x == 0, av
        if op == "ABS":
            return np.abs(x), av
        if op == "BIT_INVERT":
            return ~x, av
        if op in ("SQRT", "CEIL", "FLOOR", "RINT"):
            return {"SQRT": np.sqrt, "CEIL": np.ceil, "FLOOR": np.floor, "RINT": np.rint}[op](x), av
        if op.startswith("CAST_TO_"):
            return x.astype(NP[result_dtype(op, t)]), av
    raise AssertionError(op)


# ------------------------------------------------------------------------------------------------ node arrays
def node_types(nodes, col_dtypes, lit_dtypes):
    """dtype code of every node, or None from the first type error on"""
    ty = []
    for kind, op, lhs, rhs in nodes:
        if kind == COLUMN:
            ty.append(col_dtypes[lhs])
        elif kind == LITERAL:
            ty.append(lit_dtypes[lhs])
        elif kind == UNARY:
            ty.append(None if ty[lhs] is None else result_dtype(AST_OPS[op], ty[lhs]))
        else:
            ok = ty[lhs] is not None and ty[lhs] == ty[rhs]
            ty.append(result_dtype(AST_OPS[op], ty[lhs]) if ok else None)
        if ty[-1] is None:
            return ty + [None] * (len(nodes) - len(ty))
    return ty


def evaluate_tree(nodes, cols, lits, n):
    """recursive evaluation of the root: cols / lits are lists of (values, validity) arrays (a literal: one element each)"""
    ty = node_types(nodes, [GX[c[0].dtype] for c in cols], [GX[l[0].dtype] for l in lits])

    def ev(i):
        kind, op, lhs, rhs = nodes[i]
        if kind == COLUMN:
            return cols[lhs]
        if kind == LITERAL:
            v, ok = lits[lhs]
            return np.repeat(v, n), np.repeat(ok, n)
        if kind == UNARY:
            a, av = ev(lhs)
            return unary_value(AST_OPS[op], ty[lhs], a, av)
        a, av = ev(lhs)
        b, bv = ev(rhs)
        return binary_value(AST_OPS[op], ty[lhs], a, av, b, bv)

    v, ok = ev(len(nodes) - 1)
    return v.astype(NP[ty[-1]]), ok


def run_plan(instrs, n_slots, cols, lits, n):
    """the accumulator machine on the instruction tuples (kind, op, src_kind, src_index, in_dtype, out_dtype); asserts that a slot
    is written before it is read and that no slot index reaches n_slots"""
    acc = None
    slots = {}
    for kind, op, src_kind, src_index, in_dtype, out_dtype in instrs:
        if kind == SPILL:
            assert src_index < n_slots
            slots[src_index] = acc
            continue
        if kind == APPLY_UNARY:
            assert GX[acc[0].dtype] == in_dtype
            acc = unary_value(AST_OPS[op], in_dtype, *acc)
        else:
            if src_kind == SRC_COLUMN:
                src = cols[src_index]
            elif src_kind == SRC_LITERAL:
                src = (np.repeat(lits[src_index][0], n), np.repeat(lits[src_index][1], n))
            else:
                assert src_index in slots, "a slot is read before it is written"
                src = slots[src_index]
            assert GX[src[0].dtype] == in_dtype
            if kind == LOAD:
                acc = src
            else:
                assert GX[acc[0].dtype] == in_dtype
                l, r = (src, acc) if kind == APPLY_REV else (acc, src)
                acc = binary_value(AST_OPS[op], in_dtype, *l, *r)
        acc = (acc[0].astype(NP[out_dtype]), acc[1])
    return acc


def expansion(nodes):
    """(instructions, slots, Strahler number) of the root when every shared node is evaluated once per parent: the planner's rule
    (the heavier child first, a leaf operand is read in place, two non-leaf children spill)"""
    instr, slots, strahler, leaf = [], [], [], []
    for kind, op, lhs, rhs in nodes:
        if kind in (COLUMN, LITERAL):
            instr.append(1), slots.append(0), strahler.append(1), leaf.append(True)
        elif kind == UNARY:
            instr.append(instr[lhs] + 1), slots.append(slots[lhs]), strahler.append(strahler[lhs]), leaf.append(False)
        else:
            strahler.append(strahler[lhs] + 1 if strahler[lhs] == strahler[rhs] else max(strahler[lhs], strahler[rhs]))
            if leaf[rhs]:
                instr.append(instr[lhs] + 1), slots.append(slots[lhs])
            elif leaf[lhs]:
                instr.append(instr[rhs] + 1), slots.append(slots[rhs])
            else:
                instr.append(instr[lhs] + instr[rhs] + 2)
                slots.append(slots[lhs] + 1 if slots[lhs] == slots[rhs] else max(slots[lhs], slots[rhs]))
            leaf.append(False)
    return instr[-1], slots[-1], strahler[-1]


# ------------------------------------------------------------------------------------------------ random node arrays
def ops_for(t):
    b = [o for o in BINARY_OPS if result_dtype(o, t) is not None]
    u = [o for o in UNARY_OPS if result_dtype(o, t) is not None]
    return b, u


def random_nodes(rng, n_ops, n_leaves, share=0.15, dtypes=DTYPES):
    """a well-typed node array of n_leaves leaves (columns and literals) and n_ops operator nodes, the last one the root:
    (nodes, col dtypes, lit dtypes).  A new node prefers operands that no parent uses yet, so most arrays are close to one tree; with
    probability `share` it takes any earlier node of the right dtype (a node under several parents).  Nodes the root does not
    reach are legal: they are typed and never evaluated."""
    nodes, ty, col_dtypes, lit_dtypes = [], [], [], []
    free = []                                                    # nodes without a parent yet
    for _ in range(n_leaves):
        t = int(rng.choice(dtypes))
        if rng.random() < 0.75 or not col_dtypes:
            col_dtypes.append(t)
            nodes.append((COLUMN, 0, len(col_dtypes) - 1, 0))
        else:
            lit_dtypes.append(t)
            nodes.append((LITERAL, 0, len(lit_dtypes) - 1, 0))
        ty.append(t)
        free.append(len(nodes) - 1)

    def pick(cands):
        return cands[int(rng.integers(len(cands)))]

    for _ in range(n_ops):
        a = pick(free) if free and rng.random() >= share else int(rng.integers(len(nodes)))
        t = ty[a]
        binary_ops, unary_ops = ops_for(t)
        cands = [i for i in free if ty[i] == t and i != a]
        if rng.random() < share:
            cands = [i for i in range(len(nodes)) if ty[i] == t]
        if cands and rng.random() < 0.75:
            b = pick(cands)
            lhs, rhs = (a, b) if rng.random() < 0.5 else (b, a)
            nodes.append((BINARY, OP[pick(binary_ops)], lhs, rhs))
            used = (a, b)
        else:
            nodes.append((UNARY, OP[pick(unary_ops)], a, 0))
            used = (a,)
        for i in used:
            if i in free:
                free.remove(i)
        ty.append(result_dtype(AST_OPS[nodes[-1][1]], t))
        free.append(len(nodes) - 1)
    return nodes, col_dtypes, lit_dtypes


def random_operand(rng, t, n, null_fraction=0.3, scalar=False):
    """(values, validity) of dtype code t: small magnitudes, zeros, negative values, and for floats a NaN and infinities"""
    m = 1 if scalar else n
    dt = np.dtype(NP[t])
    if t == BOOL8:
        v = rng.integers(0, 2, m).astype(np.bool_)
    elif dt.kind == "f":
        v = np.round(rng.normal(0, 4, m), 2).astype(dt)
        if not scalar and n >= 8:
            v[rng.integers(0, n, 3)] = [np.nan, np.inf, -0.0]
    else:
        lo = -7 if dt.kind == "i" else 0
        v = rng.integers(lo, 9, m).astype(dt)
        if not scalar and n >= 8:
            info = np.iinfo(dt)
            v[rng.integers(0, n, 2)] = [info.min, info.max]
    ok = rng.random(m) >= null_fraction
    return v, ok
