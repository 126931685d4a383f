"""Element-wise operations (gx_binary_op, gx_cast) against the yardsticks each should be held to.

One process, outputs preallocated.  The arms of a case are warmed up, then timed in ROUNDS alternating rounds of REPS repetitions
each between device events; the figure of an arm is the median of its rounds.  Every case has three arms in the same run:
  copy          gx_copy_bytes of the case's algorithmic bytes (every operand read once, the output written once, bitmaps included)
  copy_if_else  gx_copy_if_else on int64 with the same rows (and the same bitmaps): the nearest kernel the library had before
  kernel        the case itself
Cases: ADD on float64 and int64, column-column and column-scalar; ADD with both bitmaps; int32 LESS int32 -> BOOL8; int8 + int8;
int32 + float64 -> float64; cast int32 -> float64.
frac = copy ms / ms.  Every output is verified outside the timed window against torch on the same buffers.

Usage: python scripts/xp/xp_binaryop.py [--rows 268435456] [--reps 20] [--rounds 5]
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
from cudf_amd.column import bitmask_words, gx_dtype, ptr, stream_ptr  # noqa: E402

lib = L.lib
ROUNDS = 5
TORCH = {"int8": torch.int8, "int32": torch.int32, "int64": torch.int64, "float64": torch.float64, "bool": torch.uint8}


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


def typed(col, dt):
    return col.data[: col.size * np.dtype(dt).itemsize].view(TORCH[dt])


def column(dt, n, seed):
    """a random column of dt; float64 as small integers in double, so that torch's sum is the same double"""
    if dt == "float64":
        c = ops.random_column(np.int64, n, seed, -(1 << 40), 1 << 40)
        typed(c, "int64").copy_(typed(c, "int64").to(torch.float64).view(torch.int64))
        c.dtype = np.dtype(np.float64)
        return c
    return ops.random_column(np.dtype(dt), n, seed)


class CieYardstick:
    """gx_copy_if_else on int64 over n rows, with both bitmaps when asked: built once per bitmap setting"""

    def __init__(self, n, nullable):
        self.lhs, self.rhs = ops.random_column(np.int64, n, 300), ops.random_column(np.int64, n, 301)
        self.mask = (ops.random_column(np.uint8, n, 302).data[:n] & 1).contiguous()
        self.lm = random_words(bitmask_words(n), 310) if nullable else None
        self.rm = random_words(bitmask_words(n), 320) if nullable else None
        self.out = torch.empty(n * 8, dtype=torch.uint8, device="cuda")
        self.out_valid = torch.zeros(bitmask_words(n), dtype=torch.int32, device="cuda") if nullable else None
        self.nulls = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.n, self.nullable = n, nullable
        self.bytes = n * 25 + (3 * n // 8 if nullable else 0)

    def __call__(self):
        L.check(lib.gx_copy_if_else(8, self.lhs.data_ptr, ptr(self.lm), 0, None, 0, self.rhs.data_ptr, ptr(self.rm), 0, None, 0, ptr(self.mask),
                                    None, 0, self.n, ptr(self.out), ptr(self.out_valid), ptr(self.nulls) if self.nullable else None, stream_ptr()),
                "gx_copy_if_else")


def binop_case(name, op, ld, rd, od, n, reps, copy_buf, cie, scalar=False, nullable=False):
    lhs = column(ld, n, 100)
    rhs = column(rd, 1 if scalar else n, 101)
    lm = random_words(bitmask_words(n), 110) if nullable else None
    rm = random_words(bitmask_words(n), 120) if nullable else None
    out = torch.empty(n * np.dtype(od).itemsize, dtype=torch.uint8, device="cuda")
    out_valid = torch.zeros(bitmask_words(n), dtype=torch.int32, device="cuda") if nullable else None
    nulls = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = stream_ptr()
    code = L.BINOP[op]

    def call():
        L.check(lib.gx_binary_op(code, gx_dtype(ld), lhs.data_ptr, ptr(lm), 0, None, 0, gx_dtype(rd), rhs.data_ptr, ptr(rm), 0, None,
                                 1 if scalar else 0, n, gx_dtype(od), ptr(out), ptr(out_valid), ptr(nulls) if nullable else None, st), "gx_binary_op")

    nbytes = n * (np.dtype(ld).itemsize + (0 if scalar else np.dtype(rd).itemsize) + np.dtype(od).itemsize) + (3 * n // 8 if nullable else 0)
    tt = compare({"copy": copy_arm(copy_buf, nbytes), "copy_if_else": cie, "kernel": call}, reps)
    a, b = typed(lhs, ld), typed(rhs, rd)
    if op == "ADD":
        want = (a.to(TORCH[od]) + b.to(TORCH[od]))
    else:
        want = (a < b).to(torch.uint8)
    ok = bool(torch.equal(want, out.view(TORCH[od])))
    if nullable:
        wb = unpack_bits(lm, n) & unpack_bits(rm, n)
        ok = ok and bool(torch.equal(unpack_bits(out_valid, n), wb)) and int(nulls.item()) == int((~wb).sum().item())
    return report(name, n, nbytes, tt, cie, ok)


def cast_case(name, sd, dd, n, reps, copy_buf, cie):
    src = column(sd, n, 130)
    out = torch.empty(n * np.dtype(dd).itemsize, dtype=torch.uint8, device="cuda")
    st = stream_ptr()

    def call():
        L.check(lib.gx_cast(gx_dtype(sd), src.data_ptr, n, gx_dtype(dd), ptr(out), st), "gx_cast")

    nbytes = n * (np.dtype(sd).itemsize + np.dtype(dd).itemsize)
    tt = compare({"copy": copy_arm(copy_buf, nbytes), "copy_if_else": cie, "kernel": call}, reps)
    ok = bool(torch.equal(typed(src, sd).to(TORCH[dd]), out.view(TORCH[dd])))
    return report(name, n, nbytes, tt, cie, ok)


def report(name, n, nbytes, tt, cie, ok):
    t_copy, t_cie, t = tt["copy"], tt["copy_if_else"], tt["kernel"]
    gbs = nbytes / t / 1e6
    print(f"{name:<40} {nbytes / n:5.2f} B/row | copy {t_copy:7.3f} ms | kernel {t:7.3f} ms ({t_copy / t:4.2f} of copy, {gbs:6.0f} GB/s) | "
          f"copy_if_else int64 {t_cie:7.3f} ms" + ("  ok" if ok else "  MISMATCH"), flush=True)
    return {"case": name, "rows": n, "bytes": nbytes, "copy_ms": round(t_copy, 3), "ms": round(t, 3), "frac_of_copy": round(t_copy / t, 3),
            "copy_if_else_ms": round(t_cie, 3), "verified": ok}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 28)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    global ROUNDS
    n, reps, ROUNDS = args.rows, args.reps, args.rounds
    torch.cuda.set_device(0)
    print(f"# xp_binaryop: {n} rows, median of {ROUNDS} alternating rounds of {reps} repetitions, {lib.gx_version().decode()}, "
          f"tile {lib.gx_elementwise_tile_rows()} rows, grid cap {lib.gx_elementwise_grid_cap()}", flush=True)
    print("# (x.xx of copy) = ms of gx_copy_bytes moving the case's algorithmic bytes (half read, half written) / ms of the kernel", flush=True)
    copy_buf = torch.zeros(n * 26 + 256, dtype=torch.uint8, device="cuda")
    rows = []
    for nullable in (False, True):
        cie = CieYardstick(n, nullable)
        tt = compare({"copy": copy_arm(copy_buf, cie.bytes), "kernel": cie}, reps)
        frac = tt["copy"] / tt["kernel"]
        print(f"{'copy_if_else int64' + (', bitmaps' if nullable else ''):<40} {cie.bytes / n:5.2f} B/row | copy {tt['copy']:7.3f} ms | kernel "
              f"{tt['kernel']:7.3f} ms ({frac:4.2f} of copy)", flush=True)
        rows.append({"case": "copy_if_else int64" + (", bitmaps" if nullable else ""), "rows": n, "bytes": cie.bytes,
                     "copy_ms": round(tt["copy"], 3), "ms": round(tt["kernel"], 3), "frac_of_copy": round(frac, 3), "verified": True})
        if not nullable:
            for name, op, ld, rd, od, scalar in (("ADD float64, column-column", "ADD", "float64", "float64", "float64", False),
                                                 ("ADD float64, column-scalar", "ADD", "float64", "float64", "float64", True),
                                                 ("ADD int64, column-column", "ADD", "int64", "int64", "int64", False),
                                                 ("ADD int64, column-scalar", "ADD", "int64", "int64", "int64", True),
                                                 ("LESS int32 int32 -> BOOL8", "LESS", "int32", "int32", "bool", False),
                                                 ("ADD int8 + int8", "ADD", "int8", "int8", "int8", False),
                                                 ("ADD int32 + float64 -> float64", "ADD", "int32", "float64", "float64", False)):
                rows.append(binop_case(name, op, ld, rd, od, n, reps, copy_buf, cie, scalar=scalar))
                torch.cuda.empty_cache()
            rows.append(cast_case("cast int32 -> float64", "int32", "float64", n, reps, copy_buf, cie))
        else:
            rows.append(binop_case("ADD int64, both bitmaps", "ADD", "int64", "int64", "int64", n, reps, copy_buf, cie, nullable=True))
        del cie
        torch.cuda.empty_cache()
    print(json.dumps({"xp": "binaryop", "rows": n, "reps": reps, "rounds": ROUNDS, "cases": rows}))
    return 0 if all(r["verified"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
