"""Row movement (gx_concatenate, gx_copy_if_else, gx_scatter) against the yardstick each should be held to.

One process, outputs preallocated.  The arms of a case (the kernel and its yardsticks) are warmed up, then timed in ROUNDS
alternating rounds of REPS repetitions each between device events; the figure of an arm is the median of its rounds.
  concatenate   8 int64 inputs into 2^28 rows: equal lengths, and odd lengths (every destination but the first misaligned against
                its source: 8-byte accesses instead of 16), each with and without bitmaps.  Yardsticks in the same run: gx_copy_bytes
                of the algorithmic bytes (rows * 16, + rows / 4 with bitmaps), and the way ops.concat_columns does it for two inputs
                stretched to eight: one device-to-device copy per input plus one gx_bitmask_copy per input ("chain").
  copy_if_else  2^28 int64 rows, the mask half true, with and without bitmaps; the copy moves rows * 25 bytes (+ 3 * rows / 8).
  scatter       2^27 int64 rows through a random permutation, next to gx_gather through the same map (the fair yardstick: the same
                bytes with the random side on the read), without bitmaps and with a source bitmap (the second pass).
frac = yardstick ms / ms.  Every output is verified outside the timed window against torch on the same buffers.

Usage: python scripts/xp/xp_copying.py [--rows 268435456] [--reps 40] [--rounds 5]
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


def compare(arms, reps, warm=3):
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


def unpack_bits(words, n):
    w = words.view(torch.int32)[: (n + 31) // 32]
    shifts = torch.arange(32, device="cuda", dtype=torch.int32)
    return ((w[:, None] >> shifts[None, :]) & 1).reshape(-1)[:n].bool()


def concat_case(name, lens, nullable, reps, copy_buf):
    n, k = sum(lens), len(lens)
    cols = [ops.random_column(np.int64, ln, 100 + i) for i, ln in enumerate(lens)]
    masks = [random_words(bitmask_words(ln), 200 + 3 * i) if nullable else None for i, ln in enumerate(lens)]
    out = torch.empty(n * 8, dtype=torch.uint8, device="cuda")
    out_valid = torch.zeros(bitmask_words(n), dtype=torch.int32, device="cuda") if nullable else None
    ptrs = (ctypes.c_void_p * k)(*[c.data.data_ptr() for c in cols])
    rows = (ctypes.c_int64 * k)(*lens)
    vp = (ctypes.c_void_p * k)(*[m.data_ptr() if m is not None else None for m in masks])
    nb = ctypes.c_size_t(0)
    st = stream_ptr()
    L.check(lib.gx_concatenate(8, k, ptrs, rows, vp, None, None, None, None, None, ctypes.byref(nb), st), "query")
    tmp = torch.empty(max(nb.value, 1), dtype=torch.uint8, device="cuda")

    def fused():
        L.check(lib.gx_concatenate(8, k, ptrs, rows, vp, None, ptr(out), ptr(out_valid), None, ptr(tmp), ctypes.byref(nb), st), "gx_concatenate")

    starts = np.concatenate([[0], np.cumsum(lens)])

    def chain():
        for i, c in enumerate(cols):
            out[starts[i] * 8: starts[i + 1] * 8].copy_(c.data[: lens[i] * 8])
            if nullable:
                L.check(lib.gx_bitmask_copy(ptr(out_valid), int(starts[i]), ptr(masks[i]), 0, lens[i], st), "gx_bitmask_copy")

    nbytes = n * 16 + (n // 4 if nullable else 0)
    t = compare({"copy": copy_arm(copy_buf, nbytes), "chain": chain, "fused": fused}, reps)
    t_copy, t_chain, t_fused = t["copy"], t["chain"], t["fused"]
    out.zero_()
    if nullable:
        out_valid.zero_()
    fused()
    want = torch.cat([c.data[: ln * 8] for c, ln in zip(cols, lens)])
    ok = bool(torch.equal(out, want))
    if nullable:
        want_bits = torch.cat([unpack_bits(m, ln) for m, ln in zip(masks, lens)])
        ok = ok and bool(torch.equal(unpack_bits(out_valid, n), want_bits))
    row = {"case": name, "rows": n, "bytes": nbytes, "copy_ms": round(t_copy, 3), "fused_ms": round(t_fused, 3), "chain_ms": round(t_chain, 3),
           "fused_frac_of_copy": round(t_copy / t_fused, 3), "chain_over_fused": round(t_chain / t_fused, 3), "verified": ok}
    print(f"concatenate {name:<22} copy {t_copy:7.3f} ms | fused {t_fused:7.3f} ({t_copy / t_fused:4.2f}) | chain {t_chain:7.3f} "
          f"({t_chain / t_fused:4.2f} x fused)" + ("  ok" if ok else "  MISMATCH"), flush=True)
    return row


def cie_case(name, n, nullable, reps, copy_buf):
    lhs, rhs = ops.random_column(np.int64, n, 300), ops.random_column(np.int64, n, 301)
    mask = (ops.random_column(np.uint8, n, 302).data[:n] & 1).contiguous()
    lm = random_words(bitmask_words(n), 310) if nullable else None
    rm = random_words(bitmask_words(n), 320) if nullable else None
    out = torch.empty(n * 8, dtype=torch.uint8, device="cuda")
    out_valid = torch.zeros(bitmask_words(n), dtype=torch.int32, device="cuda") if nullable else None
    nulls = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = stream_ptr()

    def call():
        L.check(lib.gx_copy_if_else(8, lhs.data_ptr, ptr(lm), 0, None, 0, rhs.data_ptr, ptr(rm), 0, None, 0, ptr(mask), None, 0, n, ptr(out),
                                    ptr(out_valid), ptr(nulls) if nullable else None, st), "gx_copy_if_else")

    nbytes = n * 25 + (3 * n // 8 if nullable else 0)
    tt = compare({"copy": copy_arm(copy_buf, nbytes), "kernel": call}, reps)
    t_copy, t = tt["copy"], tt["kernel"]
    pick = mask.bool()
    a, b = lhs.data[: n * 8].view(torch.int64), rhs.data[: n * 8].view(torch.int64)
    ok = bool(torch.equal(torch.where(pick, a, b), out.view(torch.int64)))
    if nullable:
        want_bits = torch.where(pick, unpack_bits(lm, n), unpack_bits(rm, n))
        ok = ok and bool(torch.equal(unpack_bits(out_valid, n), want_bits)) and int(nulls.item()) == int((~want_bits).sum().item())
    print(f"copy_if_else {name:<21} copy {t_copy:7.3f} ms | {t:7.3f} ({t_copy / t:4.2f})" + ("  ok" if ok else "  MISMATCH"), flush=True)
    return {"case": name, "rows": n, "bytes": nbytes, "copy_ms": round(t_copy, 3), "ms": round(t, 3), "frac_of_copy": round(t_copy / t, 3),
            "verified": ok}


def scatter_case(name, n, nullable, reps):
    src = ops.random_column(np.int64, n, 400)
    perm = torch.randperm(n, device="cuda", dtype=torch.int32)
    sm = random_words(bitmask_words(n), 410) if nullable else None
    target = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
    tv = torch.full((bitmask_words(n),), -1, dtype=torch.int32, device="cuda") if nullable else None
    gout = torch.empty(n * 8, dtype=torch.uint8, device="cuda")
    gv = torch.zeros(bitmask_words(n), dtype=torch.int32, device="cuda") if nullable else None
    st = stream_ptr()

    def scatter():
        if nullable:
            tv.fill_(-1)   # a bit already in place costs no atomic: every repetition starts from the all-valid target
        L.check(lib.gx_scatter(8, src.data_ptr, ptr(sm), 0, None, 0, ptr(perm), n, ptr(target), ptr(tv), n, st), "gx_scatter")

    def gather():
        L.check(lib.gx_gather(8, src.data_ptr, ptr(sm), n, ptr(perm), n, 0, ptr(gout), ptr(gv), st), "gx_gather")

    tt = compare({"gather": gather, "scatter": scatter}, max(reps // 4, 3))
    t_g, t_s = tt["gather"], tt["scatter"]
    x = src.data[: n * 8].view(torch.int64)
    want = torch.empty(n, dtype=torch.int64, device="cuda")
    want[perm.long()] = x
    ok = bool(torch.equal(want, target.view(torch.int64)))
    if nullable:
        wb = torch.empty(n, dtype=torch.bool, device="cuda")
        wb[perm.long()] = unpack_bits(sm, n)
        ok = ok and bool(torch.equal(unpack_bits(tv, n), wb))
    print(f"scatter {name:<26} gather {t_g:7.3f} ms | scatter {t_s:7.3f} ({t_g / t_s:4.2f})" + ("  ok" if ok else "  MISMATCH"), flush=True)
    return {"case": name, "rows": n, "gather_ms": round(t_g, 3), "scatter_ms": round(t_s, 3), "frac_of_gather": round(t_g / t_s, 3), "verified": ok}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 28)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    global ROUNDS
    n, reps, ROUNDS = args.rows, args.reps, args.rounds
    torch.cuda.set_device(0)
    print(f"# xp_copying: {n} rows ({n // 2} for scatter), median of {ROUNDS} alternating rounds of {reps} repetitions ({max(reps // 4, 3)} for scatter), {lib.gx_version().decode()}, "
          f"concatenate tile {lib.gx_concat_tile_rows()} rows", flush=True)
    print("# (x.xx) = yardstick ms / ms: the copy moving the case's algorithmic bytes (half read, half written), gx_gather for scatter", flush=True)
    copy_buf = torch.zeros(n * 26 + 256, dtype=torch.uint8, device="cuda")
    e = n // 8
    odd = [e + 1, e - 3, e + 5, e - 7, e + 9, e - 11, e + 13, e - 7]
    rows = []
    for name, lens, nullable in (("8 equal", [e] * 8, False), ("8 equal, bitmaps", [e] * 8, True), ("8 odd", odd, False),
                                 ("8 odd, bitmaps", odd, True)):
        rows.append(concat_case(name, lens, nullable, reps, copy_buf))
        torch.cuda.empty_cache()
    for name, nullable in (("half true", False), ("half true, bitmaps", True)):
        rows.append(cie_case(name, n, nullable, reps, copy_buf))
        torch.cuda.empty_cache()
    del copy_buf
    torch.cuda.empty_cache()
    for name, nullable in (("random permutation", False), ("random permutation, bitmap", True)):
        rows.append(scatter_case(name, n // 2, nullable, reps))
        torch.cuda.empty_cache()
    print(json.dumps({"xp": "copying", "rows": n, "reps": reps, "rounds": ROUNDS, "cases": rows}))
    return 0 if all(r["verified"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
