"""Making and reshaping columns (gx_reshape.hip) against the yardsticks each entry point should be held to.

One process, outputs preallocated.  The arms of a case are warmed up, then timed in ROUNDS alternating rounds of REPS repetitions
each between device events; the figure of an arm is the median of its rounds.  Device time at the C-ABI call.  Every case has two
arms in the same run:
  copy    gx_copy_bytes of the case's algorithmic bytes (every operand read once, the output written once)
  kernel  the case itself
and the interleave of 2 / 8 / 16 columns a third, the naive way to the same column before gx_interleave: ncols launches of
gx_scatter, column j through the strided map i -> i * ncols + j (the maps are built outside the timed window and not counted in
its bytes).  The repeat with a count column times gx_repeat_map + gx_gather for uniform counts 0..7 and for one heavy row that holds
half of the output, side by side: their ratio is the evidence for "skew does not move the cost".
Cases, int64, `--rows` output rows: interleave of 2, 8, 16 columns and of 4096 columns x rows / 4096; tile of 1000 and of 2^20 rows;
repeat_each count 4; repeat_map + gather (uniform, heavy); sequence; fill_range.
frac = copy ms / ms.  Every output is verified outside the timed window against torch on the same buffers.

Usage: python scripts/xp/xp_reshape.py [--rows 268435456] [--reps 10] [--rounds 5]
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
from cudf_amd.column import ptr, stream_ptr  # noqa: E402

lib = L.lib
ROUNDS = 5


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


def report(name, rows, nbytes, tt, ok, extra=None):
    t_copy, t = tt["copy"], tt["kernel"]
    line = (f"{name:<46} {nbytes / rows:5.2f} B/row | copy {t_copy:7.3f} ms | kernel {t:7.3f} ms ({t_copy / t:4.2f} of copy, "
            f"{nbytes / t / 1e6:6.0f} GB/s)")
    row = {"case": name, "rows": rows, "bytes": nbytes, "copy_ms": round(t_copy, 3), "ms": round(t, 3), "frac_of_copy": round(t_copy / t, 3),
           "verified": ok}
    for k, v in tt.items():
        if k not in ("copy", "kernel"):
            line += f" | {k} {v:7.3f} ms ({v / t:4.2f} x the kernel)"
            row[k + "_ms"] = round(v, 3)
    if extra:
        row.update(extra)
        line += " | " + ", ".join(f"{k} {v}" for k, v in extra.items())
    print(line + ("  ok" if ok else "  MISMATCH"), flush=True)
    return row


def random_i64(n, seed):
    out = torch.empty(n, dtype=torch.int64, device="cuda")
    L.check(lib.gx_fill_random(L.INT64, ptr(out), n, seed, 0, 0, stream_ptr()), "gx_fill_random")
    return out


def interleave_case(total, ncols, reps, copy_buf, src, out, naive):
    nrows = total // ncols
    n = nrows * ncols
    st = stream_ptr()
    ptrs = (ctypes.c_void_p * ncols)(*[src.data_ptr() + j * nrows * 8 for j in range(ncols)])
    nb = ctypes.c_size_t(0)
    args = (8, ncols, ptrs, None, None, nrows, ptr(out), None, None)
    L.check(lib.gx_interleave(*args, None, ctypes.byref(nb), None), "query")
    tmp = torch.empty(max(nb.value, 16), dtype=torch.uint8, device="cuda")
    arms = {"copy": copy_arm(copy_buf, 16 * n),
            "kernel": lambda: L.check(lib.gx_interleave(*args, ptr(tmp), ctypes.byref(nb), st), "gx_interleave")}
    maps = None
    if naive:
        maps = (torch.arange(nrows, dtype=torch.int32, device="cuda")[None, :] * ncols +
                torch.arange(ncols, dtype=torch.int32, device="cuda")[:, None]).contiguous()

        def scatter_all():
            for j in range(ncols):
                L.check(lib.gx_scatter(8, ctypes.c_void_p(ptrs[j]), None, 0, None, 0, ctypes.c_void_p(maps.data_ptr() + j * nrows * 4), nrows,
                                       ptr(out), None, n, st), "gx_scatter")
        arms["gx_scatter x ncols"] = scatter_all
    tt = compare(arms, reps)
    out[:n].zero_()
    arms["kernel"]()
    torch.cuda.synchronize()
    ok = bool(torch.equal(out[:n].view(nrows, ncols).t(), src[:n].view(ncols, nrows)))
    del maps
    return report(f"interleave {ncols} columns x {nrows} rows", n, 16 * n, tt, ok, {"scratch_bytes": nb.value})


def tile_repeat_case(total, fn, name, nrows, count, reps, copy_buf, src, out):
    n = nrows * count
    st = stream_ptr()
    arms = {"copy": copy_arm(copy_buf, 8 * n + 8 * nrows),
            "kernel": lambda: L.check(fn(8, ptr(src), None, 0, nrows, count, ptr(out), None, None, st), name)}
    tt = compare(arms, reps)
    out[:n].zero_()
    arms["kernel"]()
    torch.cuda.synchronize()
    if name == "gx_tile":
        ok = bool(torch.equal(out[:n].view(count, nrows), src[:nrows][None, :].expand(count, nrows)))
    else:
        ok = bool(torch.equal(out[:n].view(nrows, count), src[:nrows][:, None].expand(nrows, count)))
    return report(f"{name[3:]} {nrows} rows x {count}", n, 8 * n + 8 * nrows, tt, ok)


def repeat_map_case(total, heavy, reps, copy_buf, src, out):
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    body = total // 2 if heavy else total
    nrows = int(body * 0.99 / 3.5)        # the total stays below `total` (mean 3.5 a row)
    counts = torch.randint(0, 8, (nrows,), device="cuda", generator=g, dtype=torch.int64)
    if heavy:
        counts[nrows // 2] = total - body
    offsets64 = torch.zeros(nrows + 1, dtype=torch.int64, device="cuda")
    offsets64[1:] = torch.cumsum(counts, 0)
    n = int(offsets64[-1].item())
    assert n <= out.numel() and n < 2**31
    offsets = offsets64.to(torch.int32)
    gmap = torch.empty(n, dtype=torch.int32, device="cuda")
    st = stream_ptr()
    nb = ctypes.c_size_t(0)
    L.check(lib.gx_repeat_map(ptr(offsets), nrows, n, ptr(gmap), None, ctypes.byref(nb), None), "query")
    tmp = torch.empty(16, dtype=torch.uint8, device="cuda")

    def run_map():
        L.check(lib.gx_repeat_map(ptr(offsets), nrows, n, ptr(gmap), ptr(tmp), ctypes.byref(nb), st), "gx_repeat_map")

    def run_gather():
        L.check(lib.gx_gather(8, ptr(src), None, nrows, ptr(gmap), n, 0, ptr(out), None, st), "gx_gather")

    def both():
        run_map()
        run_gather()

    nbytes = 4 * (nrows + 1) + 4 * n + 4 * n + 8 * nrows + 8 * n      # offsets in, map out; map in, rows in, rows out
    arms = {"copy": copy_arm(copy_buf, nbytes), "kernel": both, "gx_repeat_map alone": run_map, "gx_gather alone": run_gather}
    tt = compare(arms, reps)
    gmap.zero_()
    both()
    torch.cuda.synchronize()
    want = torch.repeat_interleave(torch.arange(nrows, device="cuda", dtype=torch.int32), counts)
    ok = bool(torch.equal(gmap, want)) and bool(torch.equal(out[:n], src[:nrows][want.long()]))
    name = "repeat_map + gather, one row holds half" if heavy else "repeat_map + gather, uniform counts 0..7"
    return report(name, n, nbytes, tt, ok, {"source_rows": nrows})


def write_case(total, name, reps, copy_buf, out, fn, check):
    arms = {"copy": copy_arm(copy_buf, 8 * total), "kernel": fn}
    tt = compare(arms, reps)
    out[:total].zero_()
    fn()
    torch.cuda.synchronize()
    return report(name, total, 8 * total, tt, bool(check()))


def main():
    global ROUNDS
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 28)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ROUNDS = a.rounds
    total = a.rows
    print(f"# xp_reshape: {total} output rows of int64, {a.reps} reps x {ROUNDS} alternating rounds, medians; device {torch.cuda.get_device_name(0)}")
    copy_buf = torch.empty(24 * total + 4096, dtype=torch.uint8, device="cuda")
    src = random_i64(total, 1)
    out = torch.empty(total + 64, dtype=torch.int64, device="cuda")
    st = stream_ptr()
    rows = []
    for k in (2, 8, 16):
        rows.append(interleave_case(total, k, a.reps, copy_buf, src, out, True))
    rows.append(interleave_case(total, 4096, a.reps, copy_buf, src, out, False))
    rows.append(tile_repeat_case(total, lib.gx_tile, "gx_tile", 1000, total // 1000, a.reps, copy_buf, src, out))
    rows.append(tile_repeat_case(total, lib.gx_tile, "gx_tile", 1 << 20, max(total >> 20, 1), a.reps, copy_buf, src, out))
    rows.append(tile_repeat_case(total, lib.gx_repeat_each, "gx_repeat_each", total // 4, 4, a.reps, copy_buf, src, out))
    uni = repeat_map_case(total, False, a.reps, copy_buf, src, out)
    hvy = repeat_map_case(total, True, a.reps, copy_buf, src, out)
    rows += [uni, hvy]
    per_row = lambda r: r["ms"] / r["rows"]          # noqa: E731
    print(f"repeat: heavy / uniform device time per output row = {per_row(hvy) / per_row(uni):.3f} "
          f"(map alone: {hvy['gx_repeat_map alone_ms'] / hvy['rows'] / (uni['gx_repeat_map alone_ms'] / uni['rows']):.3f})", flush=True)
    init = torch.tensor([5], dtype=torch.int64, device="cuda")
    step = torch.tensor([3], dtype=torch.int64, device="cuda")
    rows.append(write_case(total, "sequence", a.reps, copy_buf, out,
                           lambda: L.check(lib.gx_sequence(L.INT64, ptr(out), total, ptr(init), ptr(step), st), "gx_sequence"),
                           lambda: torch.equal(out[:total], 5 + 3 * torch.arange(total, device="cuda", dtype=torch.int64))))
    rows.append(write_case(total, "fill_range", a.reps, copy_buf, out,
                           lambda: L.check(lib.gx_fill_range(8, ptr(out), 1, total - 1, ptr(init), st), "gx_fill_range"),
                           lambda: bool((out[1: total - 1] == 5).all()) and int(out[0]) == 0 and int(out[total - 1]) == 0))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0 if all(r["verified"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
