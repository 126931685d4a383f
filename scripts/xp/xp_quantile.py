"""Order statistics of an unsorted column (gx_quantile, gx_quantile.hip): the select path against the sort path, against the sort the
parent commit needs for the same answer, and against a copy of equal bytes.

One process, outputs and scratch preallocated.  The arms of a case are warmed up, then timed in ROUNDS alternating rounds of REPS
repetitions each between device events; the figure of an arm is the median of its rounds.  Device time at the C-ABI call -- for
gx_quantile that includes the one read-back of the plan (the call waits for the stream there), which is part of what a caller pays.
Arms of every case, in the same run:
  copy          gx_copy_bytes of the column's bytes (n elements read + n written: two of the select path's three reads, roughly)
  sort_keys     gx_sort_keys of the column (of the compacted valid rows' worth when there is a bitmap: the column itself)
  select q1/q5  gx_quantile FORCE_SELECT for q = {0.5} / {0.01, 0.25, 0.5, 0.75, 0.99}
  sort q1/q5    gx_quantile FORCE_SORT for the same
  auto q5       gx_quantile AUTO with the shipped thresholds; the path it took is printed
Cases, `--rows` rows: int64 uniform over the full range; int64 keys in [100, 10001); int64 lognormal; float64 N(0, 1); keys in
[100, 10001) with one outlier at each end (must take the fallback in AUTO); int64 uniform with validity 0.5.
Every select result is verified outside the timed window against the sort path's (bit for bit, elements and doubles).

Usage: python scripts/xp/xp_quantile.py [--rows 268435456] [--reps 5] [--rounds 5]
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
Q1 = [0.5]
Q5 = [0.01, 0.25, 0.5, 0.75, 0.99]


def compare(arms, reps, warm=2):
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


class Quantile:
    """one preallocated gx_quantile call"""

    def __init__(self, dtype, data, valid, n, qs, mode, tmp):
        self.nq = len(qs)
        self.q = (ctypes.c_double * self.nq)(*qs)
        self.f64 = torch.zeros(self.nq, dtype=torch.float64, device="cuda")
        self.elems = torch.zeros(2 * self.nq, dtype=torch.int64, device="cuda")
        self.nvalid = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.path = ctypes.c_int(0)
        self.args = (dtype, ptr(data), ptr(valid), 0, n, self.q, self.nq, L.INTERP["linear"], L.QUANTILE_MODE[mode], ptr(self.f64),
                     ptr(self.elems), ptr(self.nvalid), ctypes.byref(self.path))
        self.tmp = tmp
        self.nb = ctypes.c_size_t(tmp.numel())

    @staticmethod
    def scratch(dtype, valid, n):
        nb = ctypes.c_size_t(0)
        q = (ctypes.c_double * 1)(0.5)
        L.check(lib.gx_quantile(dtype, None, ptr(valid), 0, n, q, 1, 0, 0, None, None, None, None, None, ctypes.byref(nb), None), "query")
        return nb.value

    def __call__(self):
        L.check(lib.gx_quantile(*self.args, ptr(self.tmp), ctypes.byref(self.nb), stream_ptr()), "gx_quantile")

    def result(self):
        self()
        st = ctypes.c_int(0)
        L.check(lib.gx_quantile_status(ptr(self.tmp), ctypes.byref(st), stream_ptr()), "gx_quantile_status")
        torch.cuda.synchronize()
        return (self.f64.cpu().numpy().view(np.uint64).tolist(), self.elems.cpu().numpy().tolist(), int(self.nvalid.item()),
                L.QUANTILE_PATH.get(self.path.value))


def case(name, dtype, data, valid, n, reps, copy_buf, sort_out, want_auto=None):
    tmp = torch.empty(Quantile.scratch(dtype, valid, n) + 256, dtype=torch.uint8, device="cuda")
    st = stream_ptr()
    nbs = ctypes.c_size_t(0)
    L.check(lib.gx_sort_keys(dtype, None, ptr(sort_out), n, 0, None, ctypes.byref(nbs), None), "sort query")
    stmp = torch.empty(nbs.value + 256, dtype=torch.uint8, device="cuda")
    calls = {f"{m} q{len(q)}": Quantile(dtype, data, valid, n, q, m, tmp) for m in ("select", "sort") for q in (Q1, Q5)}
    calls["auto q5"] = Quantile(dtype, data, valid, n, Q5, "auto", tmp)
    half = (8 * n) // 64 * 64
    arms = {"copy": lambda: L.check(lib.gx_copy_bytes(ptr(copy_buf), ctypes.c_void_p(copy_buf.data_ptr() + half), half, st), "gx_copy_bytes"),
            "sort_keys": lambda: L.check(lib.gx_sort_keys(dtype, ptr(data), ptr(sort_out), n, 0, ptr(stmp), ctypes.byref(nbs), st), "gx_sort_keys")}
    arms.update(calls)
    tt = compare(arms, reps)
    res = {k: c.result() for k, c in calls.items()}
    ok = res["select q1"][:3] == res["sort q1"][:3] and res["select q5"][:3] == res["sort q5"][:3] and res["auto q5"][:3] == res["sort q5"][:3]
    auto_path = res["auto q5"][3]
    if want_auto is not None:
        ok = ok and auto_path == want_auto
    line = f"{name:<44} " + " | ".join(f"{k} {v:7.3f}" for k, v in tt.items())
    line += (f" | ms; select q1 = {tt['sort_keys'] / tt['select q1']:5.2f} x faster than sort_keys, {tt['select q1'] / tt['copy']:4.2f} copies; "
             f"paths: select {res['select q5'][3]}, auto {auto_path}")
    print(line + ("  ok" if ok else "  MISMATCH"), flush=True)
    row = {"case": name, "rows": n, "verified": ok, "auto_path": auto_path, "select_path": res["select q5"][3]}
    row.update({k.replace(" ", "_") + "_ms": round(v, 3) for k, v in tt.items()})
    del tmp, stmp
    return row


def main():
    global ROUNDS
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 28)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    ROUNDS = a.rounds
    n = a.rows
    mr, sh = ctypes.c_int64(0), ctypes.c_double(0)
    lib.gx_quantile_get_thresholds(ctypes.byref(mr), ctypes.byref(sh))
    print(f"# xp_quantile: {n} rows, {a.reps} reps x {ROUNDS} alternating rounds, medians of device ms; AUTO thresholds min_rows {mr.value}, "
          f"max_share {sh.value}; device {torch.cuda.get_device_name(0)}")
    copy_buf = torch.empty(16 * n + 4096, dtype=torch.uint8, device="cuda")
    sort_out = torch.empty(n + 64, dtype=torch.int64, device="cuda")
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    rows = []
    data = torch.empty(n, dtype=torch.int64, device="cuda")
    L.check(lib.gx_fill_random(L.INT64, ptr(data), n, 1, 0, 0, stream_ptr()), "gx_fill_random")
    rows.append(case("int64 uniform, full range", L.INT64, data, None, n, a.reps, copy_buf, sort_out))
    valid = torch.randint(-2**31, 2**31 - 1, ((n + 31) // 32 + 16,), device="cuda", generator=g, dtype=torch.int64).to(torch.int32)
    rows.append(case("int64 uniform, validity 0.5", L.INT64, data, valid, n, a.reps, copy_buf, sort_out))
    del valid
    data.random_(100, 10001, generator=g)
    rows.append(case("int64 keys in [100, 10001)", L.INT64, data, None, n, a.reps, copy_buf, sort_out))
    data[n // 3] = -2**63
    data[2 * (n // 3)] = 2**63 - 1
    rows.append(case("keys in [100, 10001) + one outlier at each end", L.INT64, data, None, n, a.reps, copy_buf, sort_out, want_auto="sort"))
    f = torch.empty(n, dtype=torch.float64, device="cuda")
    f.log_normal_(0.0, 2.0, generator=g)
    torch.mul(f, 1e6, out=f)
    data.copy_(f)
    rows.append(case("int64 lognormal (sigma 2) x 1e6", L.INT64, data, None, n, a.reps, copy_buf, sort_out))
    f.normal_(0.0, 1.0, generator=g)
    rows.append(case("float64 N(0, 1)", L.FLOAT64, f, None, n, a.reps, copy_buf, sort_out))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(rows, fh, indent=1)
    return 0 if all(r["verified"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
