"""Deduplicating selectors (gx_select_distinct KEEP_ANY / KEEP_FIRST, gx_select_unique KEEP_FIRST) on one int64 key column, against
two yardsticks measured in the same run: a device-to-device copy of the key column's bytes (gx_copy_bytes: n * 8 read + n * 8
written), and the nearest equivalent of the tree before this feature, gx_groupby_min_max(keys, row-number column) -- the LDS-partitioned
hash groupby, whose MIN / MAX per key are the first / last row of every class.

One process, warm-up, device events around REPS repetitions of the selector alone (memset of the table + insert + scan [+ resolve]);
scratch and outputs are preallocated and the host read of the count is outside the window.  Every timed result is verified once,
outside the window: the three counts against each other and against the groupby's number of groups / torch's adjacent difference.

Usage: python scripts/xp/xp_distinct.py [--rows 100000000] [--reps 10]
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
from cudf_amd import ops  # noqa: E402
from cudf_amd.column import Column, ptr, stream_ptr  # noqa: E402

lib = L.lib


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def make_keys(n, ndistinct, seed):
    """n int64 keys out of ndistinct values that look random in every bit: ids (random below ndistinct, or 0 .. n - 1 when every row
    is to be distinct) through the splitmix64 finaliser, a bijection"""
    if ndistinct >= n:
        ids = torch.arange(n, dtype=torch.int64, device="cuda")
        col = Column(ids.view(torch.uint8), np.dtype(np.int64), n)
    else:
        col = ops.random_column(np.int64, n, seed, 0, ndistinct)
    L.check(lib.gx_mix64_inplace(col.data_ptr, n, stream_ptr()), "gx_mix64_inplace")
    return col


def selector(fn, keys, n, keep, flags=3):
    """(callable that enqueues the selector, count tensor, scratch)"""
    dts = (ctypes.c_int * 1)(keys.gx)
    cols = (ctypes.c_void_p * 1)(keys.data_ptr.value)
    nb = ctypes.c_size_t(0)
    L.check(fn(1, dts, cols, None, None, n, keep, flags, None, None, ctypes.byref(nb), None), "scratch query")
    tmp = torch.empty(nb.value, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = stream_ptr()

    def run():
        L.check(fn(1, dts, cols, None, None, n, keep, flags, ptr(cnt), ptr(tmp), ctypes.byref(nb), st), "selector")

    return run, cnt, tmp


def run_case(n, ndistinct, reps, copy_buf):
    keys = make_keys(n, ndistinct, 4242)
    st = stream_ptr()
    row = {"rows": n, "value_range": ndistinct}
    counts = {}
    for name, fn, keep in (("distinct_any", lib.gx_select_distinct, L.KEEP_ANY), ("distinct_first", lib.gx_select_distinct, L.KEEP_FIRST),
                           ("unique_first", lib.gx_select_unique, L.KEEP_FIRST)):
        run, cnt, tmp = selector(fn, keys, n, keep)
        row[name + "_ms"] = round(timed(run, reps), 3)
        row[name + "_scratch_mb"] = round(tmp.numel() / 2**20, 1)
        counts[name] = int(cnt.item())
        del run, cnt, tmp
        torch.cuda.empty_cache()
    # the yardsticks
    nbytes = n * 8
    row["copy_ms"] = round(timed(lambda: L.check(lib.gx_copy_bytes(ptr(copy_buf), ctypes.c_void_p(copy_buf.data_ptr() + nbytes), nbytes, st),
                                                  "gx_copy_bytes"), reps), 3)
    rows = Column.empty(np.int32, n)
    L.check(lib.gx_sequence_i32(rows.data_ptr, n, 0, st), "gx_sequence_i32")
    max_groups = min(n, ndistinct)
    ok = Column.empty(np.int64, max_groups)
    omin, omax, ocv = Column.empty(np.int32, max_groups), Column.empty(np.int32, max_groups), Column.empty(np.int32, max_groups)
    ng = torch.zeros(1, dtype=torch.int64, device="cuda")
    nb = ctypes.c_size_t(0)
    args = (keys.gx, keys.data_ptr, None, L.INT32, rows.data_ptr, None, n, max_groups, ok.data_ptr, omin.data_ptr, omax.data_ptr, ocv.data_ptr, ptr(ng))
    L.check(lib.gx_groupby_min_max(*args, None, ctypes.byref(nb), None), "groupby query")
    gtmp = torch.empty(max(nb.value, 1), dtype=torch.uint8, device="cuda")
    row["groupby_min_max_ms"] = round(timed(lambda: L.check(lib.gx_groupby_min_max(*args, ptr(gtmp), ctypes.byref(nb), st), "gx_groupby_min_max"), reps), 3)
    groups = int(ng.item())
    # verification, outside the timed windows
    k = keys.data[: n * 8].view(torch.int64)
    runs = int((k[1:] != k[:-1]).sum().item()) + 1
    ok_all = counts["distinct_any"] == counts["distinct_first"] == groups and counts["unique_first"] == runs
    row.update({"distinct": counts["distinct_any"], "runs": runs, "groupby_groups": groups, "verified": bool(ok_all)})
    for name in ("distinct_any", "distinct_first", "unique_first"):
        row[name + "_rows_per_s"] = round(n / (row[name + "_ms"] * 1e-3), 0)
    print(f"value range {ndistinct:>11,d} ({row['distinct']:>11,d} distinct): distinct ANY {row['distinct_any_ms']:8.3f} ms  FIRST "
          f"{row['distinct_first_ms']:8.3f} ms  unique FIRST {row['unique_first_ms']:7.3f} ms  | copy {row['copy_ms']:6.3f} ms  "
          f"groupby_min_max {row['groupby_min_max_ms']:8.3f} ms  | ANY / copy {row['distinct_any_ms'] / row['copy_ms']:6.1f} x  "
          f"ANY / groupby {row['distinct_any_ms'] / row['groupby_min_max_ms']:5.2f} x  {'ok' if ok_all else 'MISMATCH'}", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    n, reps = args.rows, max(args.reps, 3)
    torch.cuda.set_device(0)
    print(f"# xp_distinct: {n} int64 rows, {reps} repetitions per timing, {lib.gx_version().decode()}", flush=True)
    print("# ms = the selector alone (table memset + insert + scan of the chunk counts [+ resolve pass]); copy = gx_copy_bytes of the key "
          "column; groupby_min_max = gx_groupby_min_max(keys, row numbers)", flush=True)
    copy_buf = torch.zeros(2 * n * 8, dtype=torch.uint8, device="cuda")
    rows = []
    for nd in (1_000, 1_000_000, 100_000_000):
        rows.append(run_case(n, nd, reps, copy_buf))
        torch.cuda.empty_cache()
    print(json.dumps({"xp": "distinct", "rows": n, "reps": reps, "cases": rows}))
    return 0 if all(r["verified"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
