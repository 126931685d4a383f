"""cudf::merge and cudf::lower_bound on one int64 key column, against two yardsticks measured in the same run: a device-to-device copy
of the merged column's bytes (gx_copy_bytes: n * 8 read + n * 8 written -- the ceiling), and what the tree offered for the job before
this feature: ops.concat_columns + ops.sort of all n rows (the only alternative).

  merge        gx_merge_order (partition + tile kernel: 8 n read, 4 n map written) + gx_gather2 of the key column through the map
               (4 n + 8 n read, 8 n written): 32 n bytes of algorithmic traffic, reported as a fraction of the copy's rate
  lower_bound  gx_search_bounds of --needles random int64 needles in the n-row merged column

One process, warm-up, device events around REPS repetitions; scratch and outputs are preallocated, nothing is read back inside a
window.  Verified once, outside the windows: the merged column equals the sorted concatenation bit for bit, the bounds equal
torch.searchsorted on a sample.

Usage: python scripts/xp/xp_merge.py [--rows 1000000000] [--needles 100000000] [--reps 5]
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


def timed(fn, reps, warm=1):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000_000, help="rows of the merged column (two sorted inputs of half that)")
    ap.add_argument("--needles", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    n, reps = args.rows, max(args.reps, 2)
    na = n // 2
    nb = n - na
    torch.cuda.set_device(0)
    st = stream_ptr()
    print(f"# xp_merge: two sorted int64 columns of {na} and {nb} rows, {args.needles} needles, {reps} repetitions per timing, "
          f"{lib.gx_version().decode()}, tile {lib.gx_merge_tile_rows()} rows", flush=True)
    a = ops.sort(ops.random_column(np.int64, na, 11))
    b = ops.sort(ops.random_column(np.int64, nb, 22))
    torch.cuda.empty_cache()

    # ---- merge: the map, then the key column through it
    dts = (ctypes.c_int * 1)(L.INT64)
    ac, bc = (ctypes.c_void_p * 1)(a.data_ptr.value), (ctypes.c_void_p * 1)(b.data_ptr.value)
    nbytes = ctypes.c_size_t(0)
    L.check(lib.gx_merge_order(1, dts, ac, None, None, na, bc, None, None, nb, None, None, None, None, ctypes.byref(nbytes), None), "scratch query")
    tmp = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
    gmap = Column.empty(np.int32, n)
    merged = Column.empty(np.int64, n)

    def run_order():
        L.check(lib.gx_merge_order(1, dts, ac, None, None, na, bc, None, None, nb, None, None, gmap.data_ptr, ptr(tmp), ctypes.byref(nbytes), st), "gx_merge_order")

    def run_gather():
        L.check(lib.gx_gather2(8, a.data_ptr, None, 0, na, b.data_ptr, None, 0, nb, gmap.data_ptr, n, merged.data_ptr, None, None, st), "gx_gather2")

    row = {"rows": n, "needles": args.needles, "merge_scratch_mb": round(nbytes.value / 2**20, 2)}
    row["merge_order_ms"] = round(timed(run_order, reps), 3)
    row["gather2_ms"] = round(timed(run_gather, reps), 3)
    row["merge_ms"] = round(row["merge_order_ms"] + row["gather2_ms"], 3)

    # ---- the ceiling: a copy of the merged column's bytes
    copy_dst = torch.empty(n * 8, dtype=torch.uint8, device="cuda")
    row["copy_ms"] = round(timed(lambda: L.check(lib.gx_copy_bytes(merged.data_ptr, ptr(copy_dst), n * 8, st), "gx_copy_bytes"), reps), 3)
    del copy_dst
    torch.cuda.empty_cache()

    # ---- the alternative of the tree before this feature: concatenate and sort again
    holder = {}

    def run_concat_sort():
        holder["out"] = ops.sort(ops.concat_columns(a, b))

    row["concat_sort_ms"] = round(timed(run_concat_sort, reps), 3)
    same = torch.equal(holder["out"].data[: n * 8].view(torch.int64), merged.data[: n * 8].view(torch.int64))
    holder.clear()
    torch.cuda.empty_cache()

    # ---- lower_bound of random needles in the merged column
    needles = ops.random_column(np.int64, args.needles, 33)
    bounds = Column.empty(np.int32, args.needles)
    hc, nc = (ctypes.c_void_p * 1)(merged.data_ptr.value), (ctypes.c_void_p * 1)(needles.data_ptr.value)

    def run_bounds():
        L.check(lib.gx_search_bounds(1, dts, hc, None, None, n, nc, None, None, args.needles, None, None, 0, bounds.data_ptr, st), "gx_search_bounds")

    row["lower_bound_ms"] = round(timed(run_bounds, reps), 3)
    m = min(args.needles, 1_000_000)
    want = torch.searchsorted(merged.data[: n * 8].view(torch.int64), needles.data[: m * 8].view(torch.int64), right=False)
    bounds_ok = torch.equal(want.to(torch.int32), bounds.data[: m * 4].view(torch.int32))

    copy_rate = 16 * n / (row["copy_ms"] * 1e-3)
    merge_rate = 32 * n / (row["merge_ms"] * 1e-3)
    row.update({
        "copy_gb_s": round(copy_rate / 1e9, 1), "merge_algorithmic_gb_s": round(merge_rate / 1e9, 1),
        "merge_fraction_of_copy_rate": round(merge_rate / copy_rate, 3),
        "merge_over_copy": round(row["merge_ms"] / row["copy_ms"], 2), "concat_sort_over_merge": round(row["concat_sort_ms"] / row["merge_ms"], 2),
        "needles_per_s": round(args.needles / (row["lower_bound_ms"] * 1e-3), 0), "verified": bool(same and bounds_ok),
    })
    print(f"merge {row['merge_ms']:9.3f} ms (map {row['merge_order_ms']:.3f} + gather {row['gather2_ms']:.3f})  | copy {row['copy_ms']:8.3f} ms  "
          f"concat + sort {row['concat_sort_ms']:9.3f} ms  | merge / copy {row['merge_over_copy']:.2f} x  concat + sort / merge "
          f"{row['concat_sort_over_merge']:.2f} x  | 32 n bytes at {row['merge_algorithmic_gb_s']:.0f} GB/s = {row['merge_fraction_of_copy_rate']:.2f} of the copy's "
          f"{row['copy_gb_s']:.0f} GB/s  | lower_bound {row['lower_bound_ms']:.3f} ms  {'ok' if row['verified'] else 'MISMATCH'}", flush=True)
    print(json.dumps({"xp": "merge", **row}))
    return 0 if row["verified"] else 1


if __name__ == "__main__":
    sys.exit(main())
