"""Fused expressions (gx_compute_column) against the chain of element-wise calls that computes the same column, and against a copy.

One process, every buffer preallocated (the chain's intermediate columns included: no allocation is timed).  The arms of a case are
warmed up, then timed in ROUNDS alternating rounds of REPS repetitions each between device events; the figure of an arm is the median
of its rounds.  Every case has three arms in the same run:
  copy    gx_copy_bytes of the fused call's algorithmic bytes (every distinct column read once, the output written once, bitmaps too)
  chain   one gx_binary_op / gx_unary_op / gx_cast call per operator node, intermediates in HBM: how the column is computed without
          the evaluator, and the baseline
  fused   gx_compute_column: one launch
Cases: a * b + c on float64 and on int32; (a > b) & (c < 5) into BOOL8; a * a + b * b; (a + b) * (c + d) (one spill); a balanced tree
of 16 leaves; a + 1 (a single node: the interpreter's overhead with nothing to win) -- each without bitmaps and with a bitmap on
every input.  speedup = chain ms / fused ms; frac = copy ms / fused ms.  The fused output is verified against the chain's outside the
timed window (valid rows bit for bit, validity words, null count).

Usage: python scripts/xp/xp_expression.py [--rows 268435456] [--reps 10] [--rounds 5]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cudf_amd import _lib as L  # noqa: E402
from cudf_amd import ast as A  # noqa: E402
from cudf_amd import ops  # noqa: E402
from cudf_amd.column import Column, bitmask_words, gx_dtype, ptr, stream_ptr  # noqa: E402

lib = L.lib
ROUNDS = 5
CHAIN_BINOP = {"NULL_EQUAL": "NULL_EQUALS"}


def compare(arms, reps, warm=2):
    """{name: median ms per call} of the arms, timed in alternating rounds in this process"""
    for fn in arms.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in arms}
    for _ in range(ROUNDS):
        for name, fn in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            ms[name].append(a.elapsed_time(b) / reps)
    return {name: float(np.median(v)) for name, v in ms.items()}


def copy_arm(copy_buf, nbytes):
    half = nbytes // 2 // 64 * 64    # a copy of B bytes moves B in all: B/2 read + B/2 written
    st = stream_ptr()
    return lambda: L.check(lib.gx_copy_bytes(ptr(copy_buf), ctypes.c_void_p(copy_buf.data_ptr() + copy_buf.numel() // 2), half, st), "gx_copy_bytes")


def random_words(nwords, seed):
    """~87 % of the bits set"""
    m = ops.random_column(np.uint32, nwords, seed).data.view(torch.int32)
    m |= ops.random_column(np.uint32, nwords, seed + 1).data.view(torch.int32)
    m |= ops.random_column(np.uint32, nwords, seed + 2).data.view(torch.int32)
    return m


def column(dt, n, seed):
    """a random column of dt; float64 as small integers in double"""
    if dt == "float64":
        c = ops.random_column(np.int64, n, seed, -(1 << 20), 1 << 20)
        v = c.data[: n * 8].view(torch.int64)
        v.copy_(v.to(torch.float64).view(torch.int64))
        c.dtype = np.dtype(np.float64)
        return c
    return ops.random_column(np.dtype(dt), n, seed, -(1 << 14), 1 << 14)


class Buf:
    """an operand of the chain: data, validity words (None: no bitmap), dtype; a literal is a scalar operand"""

    def __init__(self, dt, data, valid=None, scalar=None):
        self.dt, self.data, self.valid, self.scalar = np.dtype(dt), data, valid, scalar


def build_chain(expr, table, masks, n):
    """(closures, result Buf, null-count tensor): one element-wise call per operator node into preallocated buffers"""
    st = stream_ptr()
    calls, memo, keep = [], {}, []
    nulls = torch.zeros(1, dtype=torch.int64, device="cuda")

    def ev(e):
        if id(e) in memo:
            return memo[id(e)]
        if isinstance(e, A.ColumnReference):
            r = Buf(table[e.index].dtype, table[e.index].data, masks[e.index])
        elif isinstance(e, A.Literal):
            val, vb = ops._device_scalar(e.value, e.dtype)
            keep.append((val, vb))
            r = Buf(e.dtype, val, None, scalar=vb)
        else:
            l = ev(e.lhs)
            out_dt = ops.expression_result_dtype([Column(None, l.dt, n)] * 2, A.Operation(e.op, A.ColumnReference(0), *([A.ColumnReference(1)] if e.rhs else [])))
            out = torch.empty(n * out_dt.itemsize, dtype=torch.uint8, device="cuda")
            if e.rhs is None:
                if e.name.startswith("CAST_TO_"):
                    calls.append(lambda l=l, out=out, od=out_dt: L.check(lib.gx_cast(gx_dtype(l.dt), ptr(l.data), n, gx_dtype(od), ptr(out), st), "gx_cast"))
                else:
                    calls.append(lambda l=l, out=out, od=out_dt, c=L.UNOP[e.name]: L.check(
                        lib.gx_unary_op(c, gx_dtype(l.dt), ptr(l.data), n, gx_dtype(od), ptr(out), st), "gx_unary_op"))
                r = Buf(out_dt, out, l.valid)
            else:
                rr = ev(e.rhs)
                nullable = l.valid is not None or rr.valid is not None
                ov = torch.zeros(bitmask_words(n), dtype=torch.int32, device="cuda") if nullable else None
                c = L.BINOP[CHAIN_BINOP.get(e.name, e.name)]
                calls.append(lambda l=l, rr=rr, out=out, ov=ov, od=out_dt, c=c, nullable=nullable: L.check(
                    lib.gx_binary_op(c, gx_dtype(l.dt), ptr(l.data), ptr(l.valid), 0, ptr(l.scalar), int(l.scalar is not None), gx_dtype(rr.dt),
                                     ptr(rr.data), ptr(rr.valid), 0, ptr(rr.scalar), int(rr.scalar is not None), n, gx_dtype(od), ptr(out),
                                     ptr(ov), ptr(nulls) if nullable else None, st), "gx_binary_op"))
                r = Buf(out_dt, out, ov)
        memo[id(e)] = r
        return r

    root = ev(expr)
    return calls, root, nulls, keep


def build_fused(expr, table, masks, n):
    nodes, used, literals = A.flatten(expr)
    node_arr = (L.ExprNode * len(nodes))(*[L.ExprNode(*nd) for nd in nodes])
    keep = [ops._device_scalar(l.value, l.dtype) for l in literals]
    col_arr = (L.ExprColumn * max(len(used), 1))(*[L.ExprColumn(table[i].data.data_ptr(), masks[i].data_ptr() if masks[i] is not None else None, 0,
                                                                table[i].gx, 0) for i in used])
    lit_arr = (L.ExprLiteral * max(len(literals), 1))(*[L.ExprLiteral(v.data_ptr(), b.data_ptr(), gx_dtype(l.dtype), 0) for l, (v, b) in zip(literals, keep)])
    out_dt = ops.expression_result_dtype(table, expr)
    nullable = any(masks[i] is not None for i in used)
    out = torch.empty(n * out_dt.itemsize, dtype=torch.uint8, device="cuda")
    ov = torch.zeros(bitmask_words(n), dtype=torch.int32, device="cuda") if nullable else None
    nulls = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = stream_ptr()

    def call():
        L.check(lib.gx_compute_column(node_arr, len(nodes), col_arr, len(used), lit_arr, len(literals), n, gx_dtype(out_dt), ptr(out), ptr(ov),
                                      ptr(nulls) if nullable else None, st), "gx_compute_column")

    nbytes = n * (sum(table[i].dtype.itemsize for i in used) + out_dt.itemsize) + (n // 8) * (sum(masks[i] is not None for i in used) + int(nullable))
    return call, Buf(out_dt, out, ov), nulls, nbytes, (keep, node_arr, col_arr, lit_arr)


def unpack_bits(words, n):
    w = words.view(torch.int32)[: (n + 31) // 32]
    shifts = torch.arange(32, device="cuda", dtype=torch.int32)
    return ((w[:, None] >> shifts[None, :]) & 1).reshape(-1)[:n].bool()


def verify(fused, f_nulls, chain, c_nulls, n):
    view = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[fused.dt.itemsize]
    a, b = fused.data.view(view), chain.data.view(view)
    if fused.valid is None:
        return chain.valid is None and bool(torch.equal(a, b))
    nw = (n + 31) // 32
    ok = bool(torch.equal(fused.valid[:nw], chain.valid[:nw])) and int(f_nulls.item()) == int(c_nulls.item())
    step = 1 << 26                       # the unpacked bits of 2^28 rows at once would be gigabytes
    for lo in range(0, n, step):
        hi = min(n, lo + step)
        bits = unpack_bits(fused.valid[lo // 32:], hi - lo)
        ok = ok and bool(torch.equal(a[lo:hi][bits], b[lo:hi][bits]))
    return ok


def case(name, expr, dts, n, reps, copy_buf, nullable):
    table = [column(dt, n, 100 + 7 * i) for i, dt in enumerate(dts)]
    masks = [random_words(bitmask_words(n), 500 + 11 * i) if nullable else None for i in range(len(dts))]
    calls, c_root, c_nulls, keep1 = build_chain(expr, table, masks, n)
    fused, f_root, f_nulls, nbytes, keep2 = build_fused(expr, table, masks, n)

    def chain():
        for f in calls:
            f()

    tt = compare({"copy": copy_arm(copy_buf, nbytes), "chain": chain, "fused": fused}, reps)
    ok = verify(f_root, f_nulls, c_root, c_nulls, n)
    label = name + (", bitmaps" if nullable else "")
    print(f"{label:<44} {nbytes / n:6.2f} B/row | copy {tt['copy']:7.3f} ms | chain ({len(calls)} launches) {tt['chain']:7.3f} ms | fused "
          f"{tt['fused']:7.3f} ms | {tt['chain'] / tt['fused']:4.2f}x the chain, {tt['copy'] / tt['fused']:4.2f} of copy, "
          f"{nbytes / tt['fused'] / 1e6:6.0f} GB/s" + ("  ok" if ok else "  MISMATCH"), flush=True)
    return {"case": label, "rows": n, "bytes": nbytes, "launches_chain": len(calls), "copy_ms": round(tt["copy"], 3), "chain_ms": round(tt["chain"], 3),
            "fused_ms": round(tt["fused"], 3), "speedup_vs_chain": round(tt["chain"] / tt["fused"], 3), "frac_of_copy": round(tt["copy"] / tt["fused"], 3),
            "verified": ok}


def balanced(op, leaves):
    while len(leaves) > 1:
        leaves = [A.Operation(op, leaves[i], leaves[i + 1]) for i in range(0, len(leaves), 2)]
    return leaves[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 28)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    global ROUNDS
    n, reps, ROUNDS = args.rows, args.reps, args.rounds
    torch.cuda.set_device(0)
    print(f"# xp_expression: {n} rows, median of {ROUNDS} alternating rounds of {reps} repetitions, {lib.gx_version().decode()}, "
          f"tile {lib.gx_expression_tile_rows()} rows, grid cap {lib.gx_expression_grid_cap()}", flush=True)
    print("# (x.xx x the chain) = ms of the element-wise calls with their intermediates in HBM / ms of gx_compute_column;", flush=True)
    print("# (x.xx of copy) = ms of gx_copy_bytes moving the fused call's algorithmic bytes (half read, half written) / ms of gx_compute_column", flush=True)
    r = [A.ColumnReference(i) for i in range(16)]
    cases = [
        ("a * b + c float64", A.Operation("ADD", A.Operation("MUL", r[0], r[1]), r[2]), ["float64"] * 3),
        ("a * b + c int32", A.Operation("ADD", A.Operation("MUL", r[0], r[1]), r[2]), ["int32"] * 3),
        ("(a > b) & (c < 5) float64 -> BOOL8", A.Operation("LOGICAL_AND", A.Operation("GREATER", r[0], r[1]),
                                                           A.Operation("LESS", r[2], A.Literal(5, np.float64))), ["float64"] * 3),
        ("a * a + b * b float64", A.Operation("ADD", A.Operation("MUL", r[0], r[0]), A.Operation("MUL", r[1], r[1])), ["float64"] * 2),
        ("(a + b) * (c + d) float64, one spill", A.Operation("MUL", A.Operation("ADD", r[0], r[1]), A.Operation("ADD", r[2], r[3])), ["float64"] * 4),
        ("balanced tree of 16 leaves float64", balanced("ADD", r[:16]), ["float64"] * 16),
        ("a + 1 float64, a single node", A.Operation("ADD", r[0], A.Literal(1, np.float64)), ["float64"]),
    ]
    copy_buf = torch.zeros(n * 8 * 17 + n // 8 * 17 + 256, dtype=torch.uint8, device="cuda")
    rows = []
    for nullable in (False, True):
        for name, expr, dts in cases:
            rows.append(case(name, expr, dts, n, reps, copy_buf, nullable))
            torch.cuda.empty_cache()
    print(json.dumps({"xp": "expression", "rows": n, "reps": reps, "rounds": ROUNDS, "cases": rows}))
    return 0 if all(x["verified"] for x in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
