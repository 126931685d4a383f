"""Rolling windows (gx_rolling_window) against a device-to-device copy of the bytes they must move.

One process, warm-up, device events around REPS repetitions, outputs preallocated.  Per case (int64 / float64 SUM, with and without a
bitmap, one grouped case with groups of about 1000 rows): the tile kernel at L = preceding + following in {2, 8, 64, 512, the span
limit + 1} (gx_rolling_set_kernel(1)), the row loop at L in {2, 8, 64} (gx_rolling_set_kernel(2)), and the yardstick: gx_copy_bytes,
in the same run, of the case's algorithmic bytes
    n * (elem in + elem out) + n / 8 out bitmap   (+ n / 8 in bitmap; + 4 n labels when grouped)
frac = copy ms / ms: the fraction of the copy's rate the kernel reaches.  One output per case is verified outside the timed window
against torch on the same buffers (window sums by cumulative sums for int64, which are exact mod 2^64).

Usage: python scripts/xp/xp_rolling.py [--rows 268435456] [--reps 20]
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
from cudf_amd.column import bitmask_words, ptr, stream_ptr  # noqa: E402

lib = L.lib


def timed(fn, reps, warm=3):
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


def windows_of(L_rows):
    """(preceding, following) with preceding + following = L_rows, trailing-heavy like DataFrame.rolling(center=True)"""
    f = (L_rows - 1) // 2
    return L_rows - f, f


def run_case(name, dtype, nullable, grouped, n, reps, copy_buf):
    dt = np.dtype(dtype)
    S = lib.gx_rolling_max_span()
    col = ops.random_column(dt, n, 1234, 0, 1000) if dt.kind != "f" else ops.random_column(dt, n, 1234)
    mask = None
    if nullable:   # ~90 % valid: the AND-free way to a random bitmap is a random byte column reinterpreted as words
        mask = ops.random_column(np.uint32, bitmask_words(n), 99).data.view(torch.int32)
        mask |= ops.random_column(np.uint32, bitmask_words(n), 98).data.view(torch.int32)
        mask |= ops.random_column(np.uint32, bitmask_words(n), 97).data.view(torch.int32)
    labels = offsets = None
    if grouped:
        keys = torch.div(torch.arange(n, device="cuda", dtype=torch.int64), 1000, rounding_mode="floor")
        from cudf_amd import Column
        kc = Column(keys.view(torch.uint8), np.int64, n)
        labels, offsets = ops.group_runs([kc])
        del keys, kc
    out = torch.empty(n * 8, dtype=torch.uint8, device="cuda")
    out_valid = torch.zeros(bitmask_words(n), dtype=torch.int32, device="cuda")
    nulls = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = stream_ptr()

    def call(p, f):
        L.check(lib.gx_rolling_window(col.gx, col.data_ptr, ptr(mask), 0, n, p, f, None, None, ptr(labels), ptr(offsets), 1, L.OP_SUM,
                                      ptr(out), ptr(out_valid), ptr(nulls), st), "gx_rolling_window")

    nbytes = n * 16 + n // 8 + (n // 8 if nullable else 0) + (4 * n if grouped else 0)
    half = nbytes // 2 // 64 * 64    # a copy of B bytes moves B in all: B/2 read + B/2 written
    t_copy = timed(lambda: L.check(lib.gx_copy_bytes(ptr(copy_buf), ctypes.c_void_p(copy_buf.data_ptr() + copy_buf.numel() // 2), half, st),
                                   "gx_copy_bytes"), reps)
    row = {"case": name, "rows": n, "bytes": nbytes, "copy_ms": round(t_copy, 3), "tile": {}, "rows_kernel": {}}
    line = f"{name:<26} copy {t_copy:7.3f} ms |"
    for kern, key, Ls in ((1, "tile", (2, 8, 64, 512, S + 1)), (2, "rows_kernel", (2, 8, 64))):
        lib.gx_rolling_set_kernel(kern)
        for Lr in Ls:
            p, f = windows_of(Lr)
            t = timed(lambda: call(p, f), reps if kern == 1 or Lr <= 8 else max(reps // 4, 3))
            row[key][str(Lr)] = {"ms": round(t, 3), "frac_of_copy": round(t_copy / t, 3)}
            line += f" {key[:4]} L={Lr}: {t:7.3f} ({t_copy / t:4.2f})"
    lib.gx_rolling_set_kernel(0)
    # verification, outside the timed window: the default choice at L = 8 (int64, no nulls, no groups: exact by cumulative sums)
    ok = True
    if dt == np.int64 and not nullable and not grouped:
        p, f = windows_of(8)
        call(p, f)
        x = col.data[: n * 8].view(torch.int64)
        cs = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(x, 0)])
        i = torch.arange(n, device="cuda")
        lo, hi = torch.clamp(i - p + 1, min=0), torch.clamp(i + f, max=n - 1)
        ok = bool(torch.equal(cs[hi + 1] - cs[lo], out.view(torch.int64))) and int(nulls.item()) == 0
        del cs, i, lo, hi
    row["verified"] = ok
    print(line + ("  ok" if ok else "  MISMATCH"), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 28)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    n, reps = args.rows, args.reps
    torch.cuda.set_device(0)
    print(f"# xp_rolling: {n} rows, {reps} repetitions per timing, {lib.gx_version().decode()}, tile {lib.gx_rolling_tile_rows()} rows, "
          f"span {lib.gx_rolling_max_span()}", flush=True)
    print("# SUM; (x.xx) = copy ms / ms, the copy moving the case's algorithmic bytes (half read, half written) in the same run", flush=True)
    copy_buf = torch.zeros(n * 21 + 256, dtype=torch.uint8, device="cuda")
    cases = [("int64", np.int64, False, False), ("float64", np.float64, False, False), ("int64 bitmap", np.int64, True, False),
             ("float64 bitmap", np.float64, True, False), ("int64 groups of 1000", np.int64, False, True)]
    rows = []
    for name, dt, nullable, grouped in cases:
        rows.append(run_case(name, dt, nullable, grouped, n, reps, copy_buf))
        torch.cuda.empty_cache()
    print(json.dumps({"xp": "rolling", "rows": n, "reps": reps, "cases": rows}))
    return 0 if all(r["verified"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
