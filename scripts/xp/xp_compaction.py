"""Row filtering (gx_select_mask -> scan -> gx_compact_column) against a device-to-device copy of the bytes it must move.

One process, warm-up, device events around REPS repetitions.  Per case: the whole pipeline (select + scan + one scatter per column,
queued back to back, outputs preallocated: the host read of the count is not in the window), its three stages apart
(gx_select_set_stages), the two scatter kernels A/B (gx_compact_set_kernel), and the yardstick: gx_copy_bytes of the case's algorithmic bytes
    n * (1 + elem * (1 + s)) + n / 4          mask byte, element read, selected writes, bits written once and read once
(per extra column of the same plan: + n * elem * (1 + s) + n / 8).  Every timed output is verified once, outside the timed window:
count and contents against torch's own boolean indexing of the same buffers.

Usage: python scripts/xp/xp_compaction.py [--rows 1000000000] [--reps 20]
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
from cudf_amd.column import ptr, stream_ptr  # noqa: E402

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


def make_mask(n, s, seed):
    """BOOL8 mask of selectivity ~s, made on the device: uniform bytes in [0, 200) compared with 200 s"""
    r = ops.random_column(np.uint8, n, seed, 0, 200)
    return ops.compare_scalar(r, "lt", int(round(200 * s)))


def run_case(name, dtype, ncols, s, n, reps, copy_buf):
    dt = np.dtype(dtype)
    e = dt.itemsize
    cols = [ops.random_column(dt, n, 1000 + 17 * k) for k in range(ncols)]
    mask = make_mask(n, s, 99)
    plan = torch.empty(lib.gx_compact_plan_bytes(n), dtype=torch.uint8, device="cuda")
    nb = ctypes.c_size_t(plan.numel())
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    outs = [torch.empty(n * e, dtype=torch.uint8, device="cuda") for _ in range(ncols)]
    st = stream_ptr()

    def select():
        L.check(lib.gx_select_mask(mask.data_ptr, None, 0, n, ptr(cnt), ptr(plan), ctypes.byref(nb), st), "gx_select_mask")

    def scatter():
        for c, o in zip(cols, outs):
            L.check(lib.gx_compact_column(e, c.data_ptr, None, 0, n, ptr(plan), ptr(o), None, None, st), "gx_compact_column")

    def whole():
        select()
        scatter()

    lib.gx_select_set_stages(3)
    lib.gx_compact_set_kernel(0)
    t_all = timed(whole, reps)
    count = int(cnt.item())
    lib.gx_select_set_stages(1)
    t_sel = timed(select, reps)
    lib.gx_select_set_stages(2)
    t_scan = timed(select, reps)   # the scan re-scans its own output: same work, the plan is rebuilt below
    lib.gx_select_set_stages(3)
    select()
    t_scat = timed(scatter, reps)
    t_kernel = {}
    for kid, kname in ((1, "direct"), (2, "staged")):      # the two scatter kernels, A/B (gx_compact_set_kernel)
        lib.gx_compact_set_kernel(kid)
        t_kernel[kname] = timed(scatter, reps)
        t_kernel["whole_" + kname] = timed(whole, reps)
    lib.gx_compact_set_kernel(0)
    scatter()                                               # what is verified below is the default kernel's output
    # verification, outside the timed window: torch's boolean indexing of the same device buffers
    tm = mask.data[:n].view(torch.bool)
    assert count == int(tm.sum().item()), (count, int(tm.sum().item()))
    tdt = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[e]
    ok = True
    for c, o in zip(cols, outs):
        ref = c.data[: n * e].view(tdt)[tm]
        ok = ok and ref.numel() == count and bool(torch.equal(ref, o[: count * e].view(tdt)))
        del ref
    sel = count / n
    nbytes = int(n * (1 + e * (1 + sel)) + n / 4) + (ncols - 1) * int(n * e * (1 + sel) + n / 8)
    half = nbytes // 2    # a copy of B bytes moves B in all: B/2 read + B/2 written
    t_copy = timed(lambda: L.check(lib.gx_copy_bytes(ptr(copy_buf), ctypes.c_void_p(copy_buf.data_ptr() + (copy_buf.numel() // 2)),
                                                      half, st), "gx_copy_bytes"), reps)
    row = {"case": name, "rows": n, "elem": e, "cols": ncols, "selectivity": round(sel, 4), "count": count, "verified": ok,
           "ms": round(t_all, 3), "select_ms": round(t_sel, 3), "scan_ms": round(t_scan, 3), "scatter_ms": round(t_scat, 3),
           "rows_per_s": round(n / (t_all * 1e-3), 0), "bytes": nbytes, "gb_per_s": round(nbytes / (t_all * 1e-3) / 1e9, 1),
           "copy_ms": round(t_copy, 3), "ratio_to_copy": round(t_copy / t_all, 3),
           "scatter_direct_ms": round(t_kernel["direct"], 3), "scatter_staged_ms": round(t_kernel["staged"], 3),
           "ms_direct": round(t_kernel["whole_direct"], 3), "ms_staged": round(t_kernel["whole_staged"], 3)}
    print(f"{name:<28} {t_all:8.3f} ms  select {t_sel:7.3f}  scan {t_scan:6.3f}  scatter {t_scat:7.3f}  | {n / t_all / 1e6:8.1f} Grows/s"
          f"  {nbytes / 1e9:6.2f} GB  copy {t_copy:7.3f} ms  ratio {t_copy / t_all:5.2f}  {'ok' if ok else 'MISMATCH'}"
          f"  [scatter direct {t_kernel['direct']:7.3f} / staged {t_kernel['staged']:7.3f}; whole {t_kernel['whole_direct']:7.3f} / "
          f"{t_kernel['whole_staged']:7.3f}]", flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000_000)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    n, reps = args.rows, max(args.reps, 20)
    torch.cuda.set_device(0)
    print(f"# xp_compaction: {n} rows, {reps} repetitions per timing, {lib.gx_version().decode()}", flush=True)
    print("# ms = select + scan + scatter(s) queued back to back; copy = gx_copy_bytes moving the same number of bytes "
          "(half read, half written); ratio = copy ms / ms", flush=True)
    cases = [("int64 s=0.01", np.int64, 1, 0.01), ("int64 s=0.5 (headline)", np.int64, 1, 0.5), ("int64 s=0.99", np.int64, 1, 0.99),
             ("int32 s=0.5", np.int32, 1, 0.5), ("int8 s=0.5", np.int8, 1, 0.5), ("4 x int64 s=0.5, one plan", np.int64, 4, 0.5)]
    biggest = (int(n * (1 + 8 * 2) + n / 4) + 3 * int(n * 16 + n / 8) + 63) // 64 * 64   # both halves 16-byte aligned
    copy_buf = torch.zeros(biggest + 64, dtype=torch.uint8, device="cuda")
    rows = []
    for name, dt, ncols, s in cases:
        rows.append(run_case(name, dt, ncols, s, n, reps, copy_buf))
        torch.cuda.empty_cache()
    print(json.dumps({"xp": "compaction", "rows": n, "reps": reps, "cases": rows}))
    return 0 if all(r["verified"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
