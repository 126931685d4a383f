"""Conditional joins (gx_conditional_join_count / _write) against the materialised chain that computes the same pairs without them.

One process.  The arms of a case are warmed up, then timed in ROUNDS alternating rounds of REPS repetitions each between device
events; the figure of an arm is the median of its rounds.  Arms:
  count    gx_conditional_join_count alone, preallocated scratch (what the *_join_size functions cost)
  join     count + write through the C ABI into preallocated outputs, no host read in between (the sizes are known from a first call)
  fused    ops.conditional_inner_join end to end: count, the host read of the sizes, the allocation, write
  chain    the only route without the feature: ops.repeat / ops.tile of every column the predicate reads and of the two row-number
           columns to n_left * n_right rows, ops.compute_column, ops.apply_boolean_mask -- end to end like `fused`, verified equal
Cases at n x n rows (default 2^14 x 2^14 = 2^28 pairs, int64): l.a < r.b (about half the pairs); the interval predicate
l.lo <= r.t & r.t < l.hi at about 1e-3; a HEAVY predicate l.a // r.b == 3; l.a < r.b with bitmaps on both columns; a semi join
where every left row matches the first right row (early exit) against one where none matches anything.  Then the interval
predicate at --big x --big rows (default 2^17, where the chain cannot run): pairs per second.  Then the shape: pairs per run R in
{2, 4, 8} x right chunk in {256, 128} through gx_conditional_join_set_shape, on the count arm of two predicates.

Usage: python scripts/xp/xp_conditional_join.py [--rows 16384] [--big 131072] [--reps 3] [--rounds 5]
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
from cudf_amd.column import Column, ptr, stream_ptr  # noqa: E402

lib = L.lib
ROUNDS = 5


def compare(arms, reps, warm=1):
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


def l(i):
    return A.ColumnReference(i, "left")


def r(i):
    return A.ColumnReference(i, "right")


class Abi:
    """one join through the C ABI with everything preallocated: count() and write() queue work and read nothing back"""

    def __init__(self, left, right, expr, kind):
        self.j = ops._ConditionalJoin(left, right, expr, kind)
        self.total, self.left_total = self.j.count()
        self.sizes = torch.zeros(2, dtype=torch.int64, device="cuda")
        self.nbytes = ctypes.c_size_t(self.j.tmp.numel())
        self.out_l = torch.empty(max(self.total, 1), dtype=torch.int32, device="cuda")
        self.out_r = torch.empty(max(self.total, 1), dtype=torch.int32, device="cuda")

    def count(self):
        L.check(lib.gx_conditional_join_count(*self.j._head(), ptr(self.sizes), ptr(self.j.tmp), ctypes.byref(self.nbytes), stream_ptr()), "count")

    def join(self):
        self.count()
        L.check(lib.gx_conditional_join_write(*self.j._head(), self.total, self.left_total, ptr(self.j.tmp), ptr(self.out_l), ptr(self.out_r),
                                              stream_ptr()), "write")


def chain(left, right, expr_one_table, used_left, used_right):
    """the pairs by materialising the grid; expr_one_table reads the repeated left columns first, then the tiled right ones"""
    nl, nr = left[0].size, right[0].size
    li = Column.from_numpy(np.arange(nl, dtype=np.int32))
    ri = Column.from_numpy(np.arange(nr, dtype=np.int32))
    grid = [ops.repeat([left[i]], nr)[0] for i in used_left] + [ops.tile([right[i]], nl)[0] for i in used_right]
    gl, gr = ops.repeat([li], nr)[0], ops.tile([ri], nl)[0]
    mask = ops.compute_column(grid, expr_one_table)
    return ops.apply_boolean_mask([gl, gr], mask)


def int_column(rng, n, lo, hi, nullable=False):
    v = rng.integers(lo, hi, n).astype(np.int64)
    return Column.from_numpy(v, rng.random(n) < 0.87) if nullable else Column.from_numpy(v)


def case(name, left, right, pair_expr, table_expr, used_left, used_right, reps, with_chain=True):
    abi = Abi(left, right, pair_expr, "inner")
    arms = {"count": abi.count, "join": abi.join, "fused": lambda: ops.conditional_inner_join(left, right, pair_expr)}
    if with_chain:
        arms["chain"] = lambda: chain(left, right, table_expr, used_left, used_right)
    tt = compare(arms, reps)
    ok = True
    if with_chain:
        fl, fr = ops.conditional_inner_join(left, right, pair_expr)
        cl, cr = chain(left, right, table_expr, used_left, used_right)
        ok = bool(torch.equal(fl.data, cl.data)) and bool(torch.equal(fr.data, cr.data)) and fl.size == abi.total
    pairs = left[0].size * right[0].size
    row = {"case": name, "n_left": left[0].size, "n_right": right[0].size, "matches": abi.total, "selectivity": abi.total / pairs,
           **{k + "_ms": round(v, 3) for k, v in tt.items()}, "count_pairs_per_s": pairs / tt["count"] * 1e3,
           "join_pairs_per_s": pairs / tt["join"] * 1e3, "verified": ok}
    line = (f"{name:<44} {left[0].size} x {right[0].size}, {abi.total} matches ({abi.total / pairs:.2e}) | count {tt['count']:8.3f} ms "
            f"({pairs / tt['count'] / 1e6:7.1f} G pairs/s) | join {tt['join']:8.3f} ms | fused {tt['fused']:8.3f} ms")
    if with_chain:
        row["speedup_vs_chain"] = tt["chain"] / tt["fused"]
        line += f" | chain {tt['chain']:9.3f} ms | {tt['chain'] / tt['fused']:6.1f}x the chain" + ("  ok" if ok else "  MISMATCH")
    print(line, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 14)
    ap.add_argument("--big", type=int, default=1 << 17)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    global ROUNDS
    n, reps, ROUNDS = args.rows, args.reps, args.rounds
    torch.cuda.set_device(0)
    tl, tr = ctypes.c_int(0), ctypes.c_int(0)
    lib.gx_conditional_join_tile(ctypes.byref(tl), ctypes.byref(tr))
    print(f"# xp_conditional_join: {n} x {n} rows, median of {ROUNDS} alternating rounds of {reps} repetitions, {lib.gx_version().decode()}, "
          f"left tile <= {tl.value}, right chunk {tr.value}, R {lib.gx_conditional_join_pairs_per_run()}, grid cap {lib.gx_conditional_join_grid_cap()}",
          flush=True)
    rng = np.random.default_rng(1)
    one = A.ColumnReference
    i64 = lambda v: A.Literal(v, np.int64)
    a, b = int_column(rng, n, 0, 1 << 20), int_column(rng, n, 0, 1 << 20)
    lo = int_column(rng, n, 0, 1 << 20)
    hi = Column.from_numpy(lo.to_numpy() + rng.integers(0, 2 * (1 << 20) // 1000, n))
    t = int_column(rng, n, 0, 1 << 20)
    d = int_column(rng, n, 1, 400)
    an, bn = int_column(rng, n, 0, 1 << 20, True), int_column(rng, n, 0, 1 << 20, True)
    interval = lambda x, y, z: A.Operation("LOGICAL_AND", A.Operation("LESS_EQUAL", x, z), A.Operation("LESS", z, y))
    heavy = lambda x, y: A.Operation("EQUAL", A.Operation("FLOOR_DIV", x, y), A.Literal(3.0, np.float64))
    rows = []
    rows.append(case("l.a < r.b", [a], [b], A.Operation("LESS", l(0), r(0)), A.Operation("LESS", one(0), one(1)), [0], [0], reps))
    rows.append(case("l.lo <= r.t & r.t < l.hi", [lo, hi], [t], interval(l(0), l(1), r(0)), interval(one(0), one(1), one(2)), [0, 1], [0], reps))
    rows.append(case("l.a // r.b == 3 (HEAVY)", [a], [d], heavy(l(0), r(0)), heavy(one(0), one(1)), [0], [0], reps))
    rows.append(case("l.a < r.b, bitmaps on both", [an], [bn], A.Operation("LESS", l(0), r(0)), A.Operation("LESS", one(0), one(1)), [0], [0], reps))
    torch.cuda.empty_cache()

    # semi: every row leaves at the first run of the program / no row ever leaves
    early = Abi([a], [b], A.Operation("GREATER_EQUAL", l(0), i64(0)), "leftsemi")
    never = Abi([a], [b], A.Operation("LESS", l(0), i64(0)), "leftsemi")
    tt = compare({"semi, every row matches at once": early.count, "semi, no row matches": never.count}, reps)
    assert early.total == n and never.total == 0
    for k, v in tt.items():
        print(f"{k:<44} {n} x {n} | mark + select {v:8.3f} ms", flush=True)
        rows.append({"case": k, "ms": round(v, 3)})

    # the size where the chain cannot run
    m = args.big
    lo2 = int_column(rng, m, 0, 1 << 30)
    hi2 = Column.from_numpy(lo2.to_numpy() + rng.integers(0, 2 * (1 << 30) // 100000, m))
    t2 = int_column(rng, m, 0, 1 << 30)
    rows.append(case("l.lo <= r.t & r.t < l.hi", [lo2, hi2], [t2], interval(l(0), l(1), r(0)), None, None, None, 1, with_chain=False))

    # the shape: R x right chunk on the count arm (the default first and last)
    shapes = []
    less_abi = Abi([a], [b], A.Operation("LESS", l(0), r(0)), "inner")
    ival_abi = Abi([lo, hi], [t], interval(l(0), l(1), r(0)), "inner")
    heavy_abi = Abi([a], [d], heavy(l(0), r(0)), "inner")
    for tr_rows in (256, 128):
        for rr in (2, 4, 8):
            assert lib.gx_conditional_join_set_shape(rr, 0, tr_rows) == 0
            tt = compare({"less": less_abi.count, "interval": ival_abi.count, "heavy": heavy_abi.count}, reps)
            print(f"shape R {rr}, right chunk {tr_rows}: count l.a < r.b {tt['less']:8.3f} ms | interval {tt['interval']:8.3f} ms | "
                  f"HEAVY {tt['heavy']:8.3f} ms", flush=True)
            shapes.append({"R": rr, "right_rows": tr_rows, **{k + "_ms": round(v, 3) for k, v in tt.items()}})
    for tl_rows in (64, 128, 256):
        assert lib.gx_conditional_join_set_shape(0, tl_rows, 0) == 0
        tt = compare({"less": less_abi.count, "interval": ival_abi.count}, reps)
        print(f"shape left tile {tl_rows} (R and chunk default): count l.a < r.b {tt['less']:8.3f} ms | interval {tt['interval']:8.3f} ms", flush=True)
        shapes.append({"left_rows": tl_rows, **{k + "_ms": round(v, 3) for k, v in tt.items()}})
    assert lib.gx_conditional_join_set_shape(0, 0, 0) == 0
    print(json.dumps({"xp": "conditional_join", "rows": n, "reps": reps, "rounds": ROUNDS, "cases": rows, "shapes": shapes}))
    return 0 if all(x.get("verified", True) for x in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
