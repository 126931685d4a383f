"""Null and value replacement (gx_replace.hip) against the yardsticks each entry point should be held to.

One process, outputs preallocated.  The arms of a case are warmed up, then timed in ROUNDS alternating rounds of REPS repetitions
each between device events; the figure of an arm is the median of its rounds.  Device time at the C-ABI call: the host read of the
null count is not part of it.  Every case has two arms in the same run:
  copy    gx_copy_bytes of the case's algorithmic bytes (every operand read once, the output written once, bitmaps included)
  kernel  the case itself
and the policy fill a third: gx_segmented_fill_nulls with a `heads` array whose single 1 is at row 0, on the same column and bitmap
-- the only way to the same result before gx_replace_nulls_policy (a scan that writes one source index per row, its read-back, a
random gather).  The scratch bytes of both are reported.
Cases, int64 / float64: replace_nulls column and scalar (validity 0.5); the policy fill PRECEDING and FOLLOWING at validity 0.5 and
0.99; replace_nans scalar; clamp; find_and_replace with 8 old values; normalize_nans_and_zeros.
frac = copy ms / ms.  Every output is verified outside the timed window against torch on the same buffers.

Usage: python scripts/xp/xp_replace.py [--rows 268435456] [--reps 10] [--rounds 5]
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


def random_valid(n, p, seed):
    """(bool tensor of n rows true with probability p, its bitmap words)"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    words = torch.zeros(bitmask_words(n), dtype=torch.int32, device="cuda")
    valid = torch.empty(n, dtype=torch.bool, device="cuda")
    step = 1 << 24
    weights = (torch.ones(32, dtype=torch.int64, device="cuda") << torch.arange(32, device="cuda")).to(torch.int64)
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        v = torch.rand(r1 - r0, device="cuda", generator=g) < p
        valid[r0:r1] = v
        pad = torch.zeros((r1 - r0 + 31) // 32 * 32, dtype=torch.int64, device="cuda")
        pad[: r1 - r0] = v
        w = (pad.view(-1, 32) * weights).sum(1)
        words[r0 // 32: r0 // 32 + w.numel()] = w.to(torch.int32)      # wraps bit 31 into the sign: the same 32 bits
    return valid, words


def unpack_bits(words, n):
    out = torch.empty(n, dtype=torch.bool, device="cuda")
    shifts = torch.arange(32, device="cuda", dtype=torch.int32)
    step = 1 << 24
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        w = words[r0 // 32: (r1 + 31) // 32]
        out[r0:r1] = ((w[:, None] >> shifts[None, :]) & 1).reshape(-1)[: r1 - r0].bool()
    return out


def i64(col, n):
    return col.data[: n * 8].view(torch.int64)


def report(name, n, nbytes, tt, ok, extra=None):
    t_copy, t = tt["copy"], tt["kernel"]
    line = (f"{name:<44} {nbytes / n:5.2f} B/row | copy {t_copy:7.3f} ms | kernel {t:7.3f} ms ({t_copy / t:4.2f} of copy, "
            f"{nbytes / t / 1e6:6.0f} GB/s)")
    row = {"case": name, "rows": n, "bytes": nbytes, "copy_ms": round(t_copy, 3), "ms": round(t, 3), "frac_of_copy": round(t_copy / t, 3),
           "verified": ok}
    if "composition" in tt:
        line += f" | segmented_fill_nulls {tt['composition']:7.3f} ms ({tt['composition'] / t:4.2f} x the kernel)"
        row["composition_ms"] = round(tt["composition"], 3)
    if extra:
        row.update(extra)
        line += " | " + ", ".join(f"{k} {v}" for k, v in extra.items())
    print(line + ("  ok" if ok else "  MISMATCH"), flush=True)
    return row


def policy_case(n, p, backward, reps, copy_buf, data):
    valid, words = random_valid(n, p, 7 + backward)
    out = torch.empty(n * 8, dtype=torch.uint8, device="cuda")
    out_valid = torch.zeros(bitmask_words(n), dtype=torch.int32, device="cuda")
    nulls = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = stream_ptr()
    nb = ctypes.c_size_t(0)
    L.check(lib.gx_replace_nulls_policy(8, data.data_ptr, ptr(words), 0, n, backward, ptr(out), ptr(out_valid), ptr(nulls), None, ctypes.byref(nb), None), "q")
    tmp = torch.empty(max(nb.value, 16), dtype=torch.uint8, device="cuda")

    def call():
        L.check(lib.gx_replace_nulls_policy(8, data.data_ptr, ptr(words), 0, n, backward, ptr(out), ptr(out_valid), ptr(nulls), ptr(tmp),
                                            ctypes.byref(nb), st), "gx_replace_nulls_policy")

    heads = torch.zeros(n, dtype=torch.uint8, device="cuda")
    heads[0] = 1
    out2 = torch.empty(n * 8, dtype=torch.uint8, device="cuda")
    out2_valid = torch.zeros(bitmask_words(n), dtype=torch.int32, device="cuda")
    nb2 = ctypes.c_size_t(0)
    L.check(lib.gx_segmented_fill_nulls(8, data.data_ptr, ptr(words), ptr(heads), n, backward, ptr(out2), ptr(out2_valid), None, ctypes.byref(nb2), None), "q")
    tmp2 = torch.empty(max(nb2.value, 16), dtype=torch.uint8, device="cuda")

    def composition():
        L.check(lib.gx_segmented_fill_nulls(8, data.data_ptr, ptr(words), ptr(heads), n, backward, ptr(out2), ptr(out2_valid), ptr(tmp2),
                                            ctypes.byref(nb2), st), "gx_segmented_fill_nulls")

    nbytes = n * 16 + 3 * (n // 8)      # the column in and out, the bitmap read twice and written once
    tt = compare({"copy": copy_arm(copy_buf, nbytes), "composition": composition, "kernel": call}, reps)
    # the model: a running max (min) over the valid row numbers
    rows = torch.arange(n, device="cuda")
    if backward:
        key = torch.where(valid, n - 1 - rows, torch.full_like(rows, -1)).flip(0)
        src = torch.cummax(key, 0).values
        src = torch.where(src < 0, src, n - 1 - src).flip(0)
    else:
        src = torch.cummax(torch.where(valid, rows, torch.full_like(rows, -1)), 0).values
    has = src >= 0
    want = i64(data, n)[src.clamp(min=0)]
    got = out.view(torch.int64)
    ok = bool(torch.equal(got[has], want[has])) and bool(torch.equal(unpack_bits(out_valid, n), has))
    ok = ok and int(nulls.item()) == int((~has).sum().item())
    ok = ok and bool(torch.equal(out2.view(torch.int64)[has], want[has])) and bool(torch.equal(unpack_bits(out2_valid, n), has))
    name = f"policy fill {'FOLLOWING' if backward else 'PRECEDING'} int64, validity {p}"
    return report(name, n, nbytes, tt, ok, {"scratch_bytes": nb.value, "composition_scratch_bytes": nb2.value})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 28)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    global ROUNDS
    n, reps, ROUNDS = args.rows, args.reps, args.rounds
    torch.cuda.set_device(0)
    print(f"# xp_replace: {n} rows, median of {ROUNDS} alternating rounds of {reps} repetitions, {lib.gx_version().decode()}, "
          f"tile {lib.gx_replace_tile_rows()} rows", flush=True)
    print("# (x.xx of copy) = ms of gx_copy_bytes moving the case's algorithmic bytes (half read, half written) / ms of the kernel", flush=True)
    copy_buf = torch.zeros(n * 25 + 256, dtype=torch.uint8, device="cuda")
    st = stream_ptr()
    data = ops.random_column(np.int64, n, 100, -50, 50)
    repl = ops.random_column(np.int64, n, 101)
    out = torch.empty(n * 8, dtype=torch.uint8, device="cuda")
    out_valid = torch.zeros(bitmask_words(n), dtype=torch.int32, device="cuda")
    nulls = torch.zeros(1, dtype=torch.int64, device="cuda")
    rows = []

    for backward in (0, 1):
        for p in (0.5, 0.99):
            rows.append(policy_case(n, p, backward, reps, copy_buf, data))
            torch.cuda.empty_cache()

    valid, words = random_valid(n, 0.5, 3)
    x = i64(data, n)

    def rn_col():
        L.check(lib.gx_replace_nulls(8, data.data_ptr, ptr(words), 0, repl.data_ptr, None, 0, None, 0, n, ptr(out), None, None, st), "gx_replace_nulls")

    nbytes = n * 24 + n // 8
    tt = compare({"copy": copy_arm(copy_buf, nbytes), "kernel": rn_col}, reps)
    ok = bool(torch.equal(out.view(torch.int64), torch.where(valid, x, i64(repl, n))))
    rows.append(report("replace_nulls int64, column, validity 0.5", n, nbytes, tt, ok))

    rvalid, rwords = random_valid(n, 0.5, 4)

    def rn_col_masks():
        L.check(lib.gx_replace_nulls(8, data.data_ptr, ptr(words), 0, repl.data_ptr, ptr(rwords), 0, None, 0, n, ptr(out), ptr(out_valid),
                                     ptr(nulls), st), "gx_replace_nulls")

    nbytes = n * 24 + 3 * (n // 8)
    tt = compare({"copy": copy_arm(copy_buf, nbytes), "kernel": rn_col_masks}, reps)
    ok = bool(torch.equal(out.view(torch.int64)[valid | rvalid], torch.where(valid, x, i64(repl, n))[valid | rvalid]))
    ok = ok and bool(torch.equal(unpack_bits(out_valid, n), valid | rvalid)) and int(nulls.item()) == int((~(valid | rvalid)).sum().item())
    rows.append(report("replace_nulls int64, column, both bitmaps", n, nbytes, tt, ok))
    del rvalid, rwords

    scalar = torch.tensor([77], dtype=torch.int64, device="cuda")

    def rn_scalar():
        L.check(lib.gx_replace_nulls(8, data.data_ptr, ptr(words), 0, ptr(scalar), None, 0, None, 1, n, ptr(out), None, None, st), "gx_replace_nulls")

    nbytes = n * 16 + n // 8
    tt = compare({"copy": copy_arm(copy_buf, nbytes), "kernel": rn_scalar}, reps)
    ok = bool(torch.equal(out.view(torch.int64), torch.where(valid, x, scalar)))
    rows.append(report("replace_nulls int64, scalar, validity 0.5", n, nbytes, tt, ok))
    del valid, words
    torch.cuda.empty_cache()

    lo, hi = torch.tensor([-10], dtype=torch.int64, device="cuda"), torch.tensor([20], dtype=torch.int64, device="cuda")

    def clamp():
        L.check(lib.gx_clamp(L.INT64, data.data_ptr, n, ptr(lo), None, None, ptr(hi), None, None, ptr(out), st), "gx_clamp")

    nbytes = n * 16
    tt = compare({"copy": copy_arm(copy_buf, nbytes), "kernel": clamp}, reps)
    rows.append(report("clamp int64", n, nbytes, tt, bool(torch.equal(out.view(torch.int64), x.clamp(-10, 20)))))

    old = torch.tensor([1, 3, 5, 7, 9, 11, 13, 1], dtype=torch.int64, device="cuda")
    new = torch.tensor([-1, -3, -5, -7, -9, -11, -13, 99], dtype=torch.int64, device="cuda")

    def find():
        L.check(lib.gx_find_and_replace(L.INT64, data.data_ptr, None, 0, n, ptr(old), ptr(new), None, 0, 8, ptr(out), None, None, st),
                "gx_find_and_replace")

    tt = compare({"copy": copy_arm(copy_buf, nbytes), "kernel": find}, reps)
    odd = (x % 2 == 1) & (x >= 1) & (x <= 13)
    rows.append(report("find_and_replace int64, 8 old values", n, nbytes, tt, bool(torch.equal(out.view(torch.int64), torch.where(odd, -x, x)))))

    f = x.to(torch.float64)
    f[x == 7] = float("nan")
    f[x == 0] = -0.0
    fill = torch.tensor([2.5], dtype=torch.float64, device="cuda")

    def nans():
        L.check(lib.gx_replace_nans(L.FLOAT64, ptr(f), None, 0, ptr(fill), None, 0, None, 1, n, ptr(out), None, None, st), "gx_replace_nans")

    tt = compare({"copy": copy_arm(copy_buf, nbytes), "kernel": nans}, reps)
    ok = bool(torch.equal(out.view(torch.int64), torch.where(x == 7, fill, f).view(torch.int64)))
    rows.append(report("replace_nans float64, scalar", n, nbytes, tt, ok))

    def norm():
        L.check(lib.gx_normalize_nans_and_zeros(L.FLOAT64, ptr(f), n, ptr(out), st), "gx_normalize_nans_and_zeros")

    tt = compare({"copy": copy_arm(copy_buf, nbytes), "kernel": norm}, reps)
    want = f.clone()
    want[x == 0] = 0.0
    rows.append(report("normalize_nans_and_zeros float64", n, nbytes, tt, bool(torch.equal(out.view(torch.int64), want.view(torch.int64)))))

    print(json.dumps({"xp": "replace", "rows": n, "reps": reps, "rounds": ROUNDS, "cases": rows}))
    return 0 if all(r["verified"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
