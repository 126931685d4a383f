#!/usr/bin/env python
"""bench.py -- BASELINE.json's metric on MI355X: rows/s + achieved HBM GB/s of the hot path.

  python bench.py --gpus N --steps K --warmup W [--workload all|sort|sorted_order|join|groupby|reduce|scan|gather]
                  [--rows R] [--full] [--dump-outputs DIR] [--cpu-baseline/--no-cpu-baseline]

A "step" is one pass of the hot path over one batch of synthetic input already resident in HBM (generated on
the device by a counter-based RNG: no PCIe traffic inside or outside the timed region).

Default (N = 1, --workload all): the headline `value` is BASELINE.json configs[1], the 1e9-row int64 radix sort
(cudf::sort), timed as K steps between barriers.  A plain run does nothing else: set-up, W warm-up steps, the K
timed steps, the result line (and the outputs under --dump-outputs).

--full: the same headline, then everything else the benchmark measures and checks.  With --workload all the SAME JSON
line carries a `sorted_order` block, a `join` block (configs[2]: 1e9-row probe x 1e8-row build inner hash join, probe
phase timed, build time reported) and a `groupby` block (configs[3]: 1e9 rows, int32 key, 1e6 groups, f64 sum +
count), each timed over its own K steps with its own `roofline`, `cpu_baseline` and a device-side correctness guard
on the timed output; the headline gets its `roofline`, `cpu_baseline` and guard as well, and `sort_robustness`,
`sorted_order_robustness` and `through_cpp` follow.

--dump-outputs DIR (sort workloads on one GPU): after the timed steps, what the last step returned to its caller as
DIR/<name>.npy in float64 -- every row up to 2^21 rows, else the rows at 2^21 seeded positions, one in each of 2^21
equal ranges.  int64 keys are split into exact halves (`sorted_keys_hi32` = key >> 32, `sorted_keys_lo32` = the low 32
bits).  The inputs are seeded, so two builds run with the same arguments can be compared file by file.

N > 1: one process per GPU (torch.distributed / RCCL over xGMI).  `python bench.py --gpus N` spawns the N ranks
itself (and fails when fewer devices are visible); under torchrun (RANK / WORLD_SIZE set) it joins the group it
was given.  Every rank holds `--rows` rows and the step is the DISTRIBUTED operator of cudf_amd/distributed.py
(range-partitioned sort / hash-partitioned join / pre-aggregated groupby: one all-to-all exchange each, no
all-reduce) -> "scaling": "weak", value = rows of all ranks / max-over-ranks time.

roofline     -- dominant kernel: algorithmic bytes per launch / average launch duration measured live with HIP
                events on the launch stream (gx_sort_profile / gx_join_profile); peak = 8.0 TB/s HBM3E.
cpu_baseline -- `value`: the reference's own CPU path (pandas sort_values / merge / groupby, kind "reference", 1 core) timed
                on the host on a bounded sample of the same workload; pyarrow (all host threads) and the oracle's C port
                (oracle/oracle.c, 1 thread: `port_rows_per_s`) beside it.
"""
import argparse
import ctypes
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec (MI355X_MICROARCH.md)
PROFILE_SLOTS = 64       # event slots of gx_sort_profile_slot / gx_join_profile_slot (include/cudf_amd/gx_knobs.h)
HBM_COPY_GBS = 6290.0   # measured copy ceiling (same guide)
METRIC = "rows/sec + achieved HBM GB/s: 1e9-row int64 sort & hash-join, 1/2/4/8 GPU"


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="all",
                    choices=["all", "sort", "sorted_order", "sorted_order_table", "sort_by_key", "join", "groupby", "groupby_minmax", "join_multikey", "groupby_multikey", "reduce", "scan", "gather"])
    ap.add_argument("--table-keys", default="lowcard", choices=["lowcard", "random", "tiny"],
                    help="sorted_order_table: lowcard = 1000 distinct leading values x random 64-bit second column (ties of the leading column by "
                         "the million); random = random 64-bit leading column (no ties); tiny = 10 x 100 distinct values (whole tuples tie)")
    ap.add_argument("--rows", type=float, default=1e9)
    ap.add_argument("--algo", type=int, default=0,
                    help="sort knob: 0 onesweep/windowed look-back, 1 three-kernel, 2 onesweep/one-tile look-back")
    ap.add_argument("--gb-algo", type=int, default=0, help="groupby knob: 0 auto, 1 global table, 2 LDS-partitioned")
    ap.add_argument("--gb-split", type=int, default=1)
    ap.add_argument("--gb-keys", default="dense", choices=["dense", "random", "random64"],
                    help="groupby: dense = int32 ids in [0, 1e6) (BASELINE config 4); random = the same ids through a 32-bit mixing bijection "
                         "(sparse int32 keys: they hash like random numbers); random64 = int64 keys, ids through the splitmix64 finalizer")
    ap.add_argument("--gb-pbits", type=int, default=0, help="groupby knob: 2^bits hash partitions; 0 (default) = 512, and 256 chosen on the device for "
                                                              "dense ids (round 4); 8 / 9 = fixed")
    ap.add_argument("--gb-dense", type=int, default=1, help="groupby knob (round 6): 1 dense ids by direct address -- id-range partitions, 10-byte (value, 16-bit remainder) rows, LDS table indexed by the remainder (default); 0 the hash path")
    ap.add_argument("--gb-spec", type=int, default=1, help="groupby knob: 1 hist-free speculative partition pass (default), 0 exact histogram pass")
    ap.add_argument("--no-partitioned-join", action="store_true", help="join: probe the table directly")
    ap.add_argument("--sort-order-map", type=int, default=1, help="sorted_order knob (round 6): 1 keys-only sort of (rank, row) words for 64-bit columns (default), 0 the round-3 pairs path")
    ap.add_argument("--sort-splitters", type=int, default=1, help="sort knob: 0 no splitter mode (uneven columns go to the LSD passes), 1 default")
    ap.add_argument("--join-probe-kernel", type=int, default=0, help="join knob: 0 pipelined tag probe on LDS-resident tags (default), 1 round-1 tag probe, 2 / 3 L2-resident direct probe (4 / 2 rows per thread)")
    ap.add_argument("--join-scatter-tile", type=int, default=0, help="join knob: rows per scatter tile (0 = default)")
    ap.add_argument("--join-xp", type=int, default=133, help="join knob (round 6; default 133): bit 0 record-form partition pass (12-byte {key, row} runs), bit 1 24576-row scatter tiles, bit 2 pipelined service wave of the probe on fixed pieces per region, bit 7 the probe with every load a trip ahead of its use + overflow list (k_pj2_probe_rare); 5 = the first round-6 cut, 0 = the round-5 kernels")
    ap.add_argument("--join-unchecked", action="store_true", help="join: skip the result guards (ablation knobs of --join-xp give wrong results by design); the line says UNCHECKED")
    ap.add_argument("--join-build-kernel", type=int, default=0, help="join knob: 0 sub-table build with the tags in LDS (default), 1 round-2 build (global CAS + k_tags)")
    ap.add_argument("--join-spec", type=int, default=1, help="join knob: 1 hist-free speculative partition (default), 0 round-2 path")
    ap.add_argument("--join-early-loads", type=int, default=0, help="join knob: bit 0 pipelined probe requests rows at the top of a trip, bit 1 deferral queue")
    ap.add_argument("--join-keys", default="random", choices=["random", "dense"],
                    help="join: random = SURVEY 8d (build = distinct random 64-bit keys, probe = 30%% drawn from them + 70%% from a "
                         "disjoint random set); dense = round 2's arithmetic progressions 3i+1 (kept for comparison)")
    ap.add_argument("--no-hybrid", action="store_true", help="sort: disable the hybrid MSD path (LSD passes only)")
    ap.add_argument("--no-cursor", action="store_true", help="sort: disable the cursor path (sampled plan + atomic-cursor partition levels); the look-back path runs")
    ap.add_argument("--sort-cell", type=int, default=0, help="sort knob: local-sort cell capacity (0 auto, 8192, 16384)")
    ap.add_argument("--sort-lbw", type=int, default=16, help="sort knob: predecessors per look-back round of the partition passes (4, 8, 16)")
    ap.add_argument("--key-range", type=int, nargs=2, default=None, metavar=("LO", "HI"),
                    help="sort: keys uniform in [LO, HI) instead of the full int64 range (the reference's own "
                         "benchmark distribution is 100 10001: benchmarks/sort/sort.cpp:24-26)")
    ap.add_argument("--hot-copies", type=float, default=0, help="sort: this many rows carry ONE value (a hot value: zeros, a sentinel)")
    ap.add_argument("--key-type", default="int64", choices=["int64", "float64"],
                    help="sort: float64 = a FLOAT64 column, keys drawn as N(0, 1) (--key-dist normal, the default for floats) or U[0, 1) (--key-dist uniform)")
    ap.add_argument("--key-dist", default="uniform", choices=["uniform", "normal", "zipf", "sorted", "lognormal", "clusters", "dupids"],
                    help="sort: distribution of the int64 keys.  normal = round(N(0, 1) * 2^40) (bell-shaped level-0 buckets); zipf = "
                         "floor(u^-5) clipped to 2^31 (the continuous form of Zipf(1.2): 18 %% of the rows carry the value 1); sorted = the "
                         "uniform keys, already in ascending order.  Robustness lines (VERDICT r3 next 3), not the headline")
    ap.add_argument("--key-copies", type=int, default=100, help="sort --key-dist dupids: rows per distinct id (ids = a 64-bit mixing bijection of [0, rows / copies): "
                                                                "wide keys WITH duplicates, a foreign-key column of hashed ids)")
    ap.add_argument("--force-sharded", action="store_true",
                    help="run the MULTI-GPU code path (pre-flight, sharded operators with the exchange forced, their guards) in a "
                         "1-rank group on one GPU: what `--gpus N` executes, testable where only one device is visible")
    ap.add_argument("--preflight-only", action="store_true", help="multi-GPU: run the oracle-checked pre-flight of the sharded operators, print its verdict as one JSON line, exit")
    ap.add_argument("--preflight-timeout", type=float, default=90.0, help="multi-GPU: seconds the watchdog gives one pre-flight operator call")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline, everything else the benchmark measures and checks: the sorted_order / join / groupby "
                         "blocks of --workload all, CPU baselines, per-kernel roofline figures, guards on the timed output, the "
                         "robustness distributions and the C++-surface ratios.  Off: set-up, warm-up, the timed steps, the result line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last step returned (sort workloads, one GPU) as DIR/<name>.npy in float64; "
                         "more than 2^21 rows: a fixed seeded sample of 2^21 of them")
    ap.add_argument("--through-cpp", dest="through_cpp", action="store_true", default=None,
                    help="also time cudf::sort / sorted_order / hash_join::inner_join / groupby::aggregate through the C++ surface "
                         "(tests/cpp/cudf_api_bench, default pooled mr) and report the ratio to the C-ABI numbers; default: on for "
                         "--full --workload all on one GPU, off otherwise")
    ap.add_argument("--no-through-cpp", dest="through_cpp", action="store_false")
    ap.add_argument("--robustness", dest="robustness", action="store_true", default=None,
                    help="sort the same 1e9 rows on other VALUE DISTRIBUTIONS (bell-shaped, lognormal, Zipf-like, two clusters, keys around zero, "
                         "the reference benchmark's [100, 10001), a hot value) and report each time and its ratio to the uniform line; "
                         "default: on for --full --workload all on one GPU")
    ap.add_argument("--no-robustness", dest="robustness", action="store_false")
    ap.add_argument("--cpu-baseline", dest="cpu", action="store_true", default=None, help="default: on with --full, off otherwise")
    ap.add_argument("--no-cpu-baseline", dest="cpu", action="store_false")
    ap.add_argument("--cpu-rows", type=float, default=0, help="rows of the CPU-baseline sample (0 = per-workload default)")
    ap.add_argument("--cpu-rows-pandas", type=float, default=0,
                    help="rows of the pandas / pyarrow legs; 0 = per-leg default: sort 1e8 and groupby 1e8 (BASELINE.md section 3's "
                         "larger size, ~15 s per library), join 1e7 (pandas.merge at 1e8 probe rows takes minutes)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if args.dump_outputs and (args.workload not in ("all", "sort", "sorted_order") or args.gpus > 1 or args.force_sharded):
        ap.error("--dump-outputs writes the output of the sort workloads (all, sort, sorted_order) on one GPU")
    if args.cpu is None:
        args.cpu = args.full
    return args


# ------------------------------------------------------------------------------------------------
# CPU baselines (rank 0, N = 1): the oracle is the checker / baseline, never the product
# ------------------------------------------------------------------------------------------------

def _cpu_line(extra, pandas_key, pandas_sample, port_rows_per_s, port_sample):
    """The cpu_baseline object.  `value` is the reference's own CPU path -- pandas, which is what a cudf user falls back to and what
    BASELINE.json's configs[0] names (north_star: "next to the reference's own CPU path (pandas/pyarrow on the GPU box's host cores, core
    count stated)") -- kind "reference", cores 1 (pandas' sort / merge / groupby kernels are single-threaded); the pyarrow figure (all host
    threads: `pyarrow_threads`) and the oracle's plain-C port on one core stand beside it.  Only when pandas is missing does the port
    become `value` (kind "port")."""
    if pandas_key in extra:
        return {"value": extra[pandas_key], "unit": "rows/s", "cores": 1, "kind": "reference",
                "sample": pandas_sample.format(m=extra.get("pandas_rows")), "host_cpus": os.cpu_count(),
                "port_rows_per_s": port_rows_per_s, "port_cores": 1, "port_sample": port_sample, **extra}
    return {"value": port_rows_per_s, "unit": "rows/s", "cores": 1, "kind": "port", "sample": port_sample, "host_cpus": os.cpu_count(), **extra}


def cpu_baseline_sort(rows, pandas_rows):
    """oracle ("port") timed on the host: single-thread LSD radix sort in C + pandas / pyarrow for context."""
    import numpy as np
    from oracle import c_oracle
    n = int(rows)
    rng = np.random.default_rng(42)
    v = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
    t0 = time.perf_counter()
    out = c_oracle.sort_i64(v)
    dt = time.perf_counter() - t0
    assert out[0] <= out[n // 2] <= out[-1]
    extra = {}
    try:
        import pandas as pd
        m = min(n, int(pandas_rows))
        df = pd.DataFrame({"a": v[:m]})
        t0 = time.perf_counter()
        df.sort_values("a", kind="stable")
        extra["pandas_sort_values_rows_per_s"] = m / (time.perf_counter() - t0)
        extra["pandas_rows"] = m
        import pyarrow as pa
        import pyarrow.compute as pc
        arr = pa.array(v[:m])
        t0 = time.perf_counter()
        pc.sort_indices(arr)
        extra["pyarrow_sort_indices_rows_per_s"] = m / (time.perf_counter() - t0)
        extra["pyarrow_threads"] = pa.cpu_count()
    except Exception as e:  # pandas is context only
        extra["pandas_error"] = repr(e)
    return _cpu_line(extra, "pandas_sort_values_rows_per_s",
                     "pandas.DataFrame.sort_values(kind='stable') on {m} uniform int64 rows (seed 42): the reference's own CPU path, BASELINE.json configs[0]",
                     n / dt, f"{n} uniform int64 rows (seed 42), oracle/oracle.c orc_sort_i64 (8-pass LSD radix, 1 thread)")


def cpu_baseline_join(rows, pandas_rows):
    import numpy as np
    from oracle import c_oracle
    n = int(rows)
    rng = np.random.default_rng(12345)
    build = rng.permutation(n // 5).astype(np.int64)[: n // 10]
    probe = rng.integers(0, n // 3, n).astype(np.int64)
    t0 = time.perf_counter()
    l, r = c_oracle.inner_join_i64(probe, build)
    dt = time.perf_counter() - t0
    extra = {}
    try:
        import pandas as pd
        m = min(n, int(pandas_rows))
        lp = pd.DataFrame({"k": probe[:m]})
        rp = pd.DataFrame({"k": build, "r": np.arange(len(build))})
        t0 = time.perf_counter()
        lp.merge(rp, on="k", how="inner")
        extra["pandas_merge_rows_per_s"] = m / (time.perf_counter() - t0)
        extra["pandas_rows"] = m
        import pyarrow as pa
        lt = pa.table({"k": probe[:m]})
        rt = pa.table({"k": build, "r": np.arange(len(build))})
        t0 = time.perf_counter()
        lt.join(rt, keys="k", join_type="inner")          # pyarrow Table.join (Acero hash join, all host threads)
        extra["pyarrow_table_join_rows_per_s"] = m / (time.perf_counter() - t0)
        extra["pyarrow_threads"] = pa.cpu_count()
    except Exception as e:  # context only
        extra["pandas_error"] = repr(e)
    extra["matches"] = int(len(l))
    return _cpu_line(extra, "pandas_merge_rows_per_s",
                     "pandas.DataFrame.merge(how='inner') of {m} probe rows x " + str(len(build)) + " build rows, int64 keys: the reference's own CPU path",
                     n / dt, f"probe {n} x build {len(build)} int64 rows, oracle/oracle.c orc_inner_join_i64 (count+retrieve)")


def cpu_baseline_groupby(rows, pandas_rows):
    import numpy as np
    from oracle import c_oracle
    n = int(rows)
    rng = np.random.default_rng(7)
    k = rng.integers(0, 1_000_000, n).astype(np.int32)
    v = rng.random(n)
    t0 = time.perf_counter()
    c_oracle.groupby_dense_sum_count(k, v, 1_000_000)
    dt = time.perf_counter() - t0
    extra = {}
    try:
        import pandas as pd
        m = min(n, int(pandas_rows))
        df = pd.DataFrame({"k": k[:m], "v": v[:m]})
        t0 = time.perf_counter()
        df.groupby("k", sort=False).agg(s=("v", "sum"), c=("v", "count"))
        extra["pandas_groupby_rows_per_s"] = m / (time.perf_counter() - t0)
        extra["pandas_rows"] = m
        import pyarrow as pa
        tb = pa.table({"k": k[:m], "v": v[:m]})
        t0 = time.perf_counter()
        tb.group_by("k").aggregate([("v", "sum"), ("v", "count")])   # pyarrow Table.group_by
        extra["pyarrow_group_by_rows_per_s"] = m / (time.perf_counter() - t0)
        extra["pyarrow_threads"] = pa.cpu_count()
    except Exception as e:  # context only
        extra["pandas_error"] = repr(e)
    return _cpu_line(extra, "pandas_groupby_rows_per_s",
                     "pandas groupby('k', sort=False).agg(sum, count) on {m} rows, 1e6 int32 groups, f64 values: the reference's own CPU path",
                     n / dt, f"{n} rows, 1e6 int32 groups, f64 sum+count, oracle/oracle.c orc_groupby_dense_sum_count")


# ------------------------------------------------------------------------------------------------
# launcher: `python bench.py --gpus N` without torchrun spawns the ranks itself
# ------------------------------------------------------------------------------------------------

def spawn_ranks(args):
    import torch
    have = torch.cuda.device_count()
    if have < args.gpus:
        print(f"bench.py: --gpus {args.gpus} but only {have} device(s) visible", file=sys.stderr)
        return 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


class Ctx:
    """what every workload needs: library handles, rank info, a barrier"""

    def __init__(self, args):
        import numpy as np
        import torch
        import torch.distributed as dist
        self.args = args
        self.rank = int(os.environ.get("RANK", "0"))
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(self.local)
        self.sharded = self.world > 1 or args.force_sharded   # the multi-GPU code path (a 1-rank group under --force-sharded)
        if self.sharded:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            if "MASTER_PORT" not in os.environ:
                with socket.socket() as so:
                    so.bind(("127.0.0.1", 0))
                    os.environ["MASTER_PORT"] = str(so.getsockname()[1])
            dist.init_process_group("nccl", rank=self.rank, world_size=self.world, device_id=torch.device("cuda", self.local))
            if args.force_sharded:
                from cudf_amd import distributed as D
                D._FORCE_EXCHANGE = True
        self.preflight = None   # verdict of the pre-flight (multi-GPU): which sharded operators passed the oracle over this transport
        self.beat = time.monotonic()
        from cudf_amd import Column, ops, _lib as L
        from cudf_amd.column import device_bytes, ptr, stream_ptr
        self.np, self.torch, self.dist = np, torch, dist
        self.Column, self.ops, self.L, self.lib = Column, ops, L, L.lib
        self.device_bytes, self.ptr = device_bytes, ptr
        self.stream = stream_ptr()
        self.n = int(args.rows)

    def barrier(self):
        self.torch.cuda.synchronize()
        if self.world > 1:
            self.dist.barrier()
        self.torch.cuda.synchronize()
        self.beat = time.monotonic()

    def timed(self, step, per_step=None, after_warmup=None, slot=None, read_slot=None):
        """W warm-ups, then exactly K steps between barriers; max over ranks.  Returns seconds per step.
        slot(k) / read_slot(): the kernels' HIP events are recorded INSIDE the timed steps, step k into event slot k % 64
        (gx_*_profile_slot, a host-side index), and read after the closing barrier -- a read-back behind every step made the host wait
        for the step and put a round trip between two timed steps (round 5 / early round 6: +0.3 ms per 11-ms step)."""
        a = self.args
        for _ in range(a.warmup):
            step()
        if after_warmup:
            after_warmup()
        self.barrier()
        t0 = time.perf_counter()
        for k in range(a.steps):
            if slot:
                slot(k % PROFILE_SLOTS)
            step()
            if per_step:
                per_step()
            self.beat = time.monotonic()
        self.barrier()
        dt = time.perf_counter() - t0
        if slot and read_slot:
            for k in range(max(0, a.steps - PROFILE_SLOTS), a.steps):   # (more steps than slots: the last 64 launches)
                slot(k % PROFILE_SLOTS)
                read_slot()
            slot(0)
        if self.world > 1:
            t = self.torch.tensor([dt], device="cuda", dtype=self.torch.float64)
            self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt / a.steps

    def as_tensor(self, col, dt):
        return col.data[: col.size * col.dtype.itemsize].view(dt)


def start_heartbeat_monitor(c, limit_s=600.0):
    """Multi-GPU runs only: a daemon thread that ends the process when the main thread has made no progress for `limit_s` seconds
    (a collective whose peer never arrived blocks for ever inside RCCL -- there is no timeout on that side).  The driver then sees
    a failed run with the reason on stderr instead of a hang; torchrun takes the other ranks down with it."""
    import threading

    def watch():
        while True:
            time.sleep(5.0)
            stale = time.monotonic() - c.beat
            if stale > limit_s:
                print(f"bench.py: rank {c.rank}: no progress for {stale:.0f} s (a collective that never completed?): giving up", file=sys.stderr, flush=True)
                os._exit(5)
    threading.Thread(target=watch, name="bench-heartbeat", daemon=True).start()


def guarded(c, what, fn, timeout_s):
    """fn() on a worker thread under a watchdog: (result, None) or (None, reason).  On a timeout the RCCL communicators of the C++
    operators are ABORTED (gxd_comm_abort -> ncclCommAbort: the blocked call returns an error); a call that does not come back
    even then ends the process -- a pre-flight can fail, it cannot hang."""
    import threading
    box = {}

    def run():
        try:
            c.torch.cuda.set_device(c.local)
            box["v"] = fn()
            c.torch.cuda.synchronize()
        except BaseException as e:  # noqa: BLE001 -- reported as the verdict
            box["e"] = e
    t = threading.Thread(target=run, name=f"preflight-{what}", daemon=True)
    t.start()
    t.join(timeout_s)
    c.beat = time.monotonic()
    if t.is_alive():
        from cudf_amd import distributed as D
        print(f"bench.py: rank {c.rank}: pre-flight {what}: no answer after {timeout_s:.0f} s -- aborting the communicator", file=sys.stderr, flush=True)
        D.abort_communicators()
        t.join(30.0)
        if t.is_alive():
            print(f"bench.py: rank {c.rank}: pre-flight {what}: still blocked after the abort: giving up", file=sys.stderr, flush=True)
            os._exit(4)
        return None, f"timeout after {timeout_s:.0f} s (communicator aborted)"
    if "e" in box:
        return None, repr(box["e"])
    return box.get("v"), None


def preflight(c):
    """BEFORE any timed step of a multi-GPU line: every rank runs the SHIPPED sharded operators -- gxd_sort
    on both of its paths, gxd_join_build + gxd_join_probe, gxd_groupby_sum_count: C++ over the RCCL transport -- on small seeded
    shards of UNEVEN sizes (one of them empty from 3 ranks on), under a watchdog; the results travel to rank 0, which regenerates
    every rank's input from its seed and compares with the CPU oracle on the concatenation (sort: bit-exact; join: the canonical
    pair set in global rows; groupby: keys, counts, sums to 1e-12).  The verdict is broadcast: an operator that failed, or did not
    answer, is timed through the torch.distributed implementation instead and the line says so.  The oracle is the checker here,
    exactly as in tests/test_gpu_distributed_loopback.py; nothing it computes is timed."""
    import numpy as np
    torch, dist = c.torch, c.dist
    from cudf_amd import distributed as D
    from cudf_amd import gxd
    W, rk = c.world, c.rank
    t_start = time.perf_counter()
    tmo = c.args.preflight_timeout

    def shard_rows(total_per_rank, r):
        if W >= 3 and r == 1:
            return 0                                   # an EMPTY shard
        return int(total_per_rank * (1 + (r % 3)) / 2)  # uneven: 0.5x / 1x / 1.5x

    def gen(r):
        rng = np.random.default_rng(9000 + r)
        d = {}
        d["sort_fused"] = rng.integers(-2**63, 2**63 - 1, shard_rows(4_000_000, r) if W > 1 else 2_600_000, dtype=np.int64)
        f = rng.standard_normal(shard_rows(400_000, r)) * 1e6
        f[::1013] = np.nan
        f[5::997] = -0.0
        d["sort_sample"] = f
        d["build"] = (rng.permutation(1_500_000)[: shard_rows(200_000, r)].astype(np.int64) * W + r) * 7919   # globally distinct
        d["probe"] = rng.integers(0, 1_500_000 * W, shard_rows(900_000, r)).astype(np.int64) * 7919
        d["gk"] = rng.integers(0, 20_000, shard_rows(700_000, r)).astype(np.int32)
        d["gv"] = rng.random(len(d["gk"]))
        return d
    mine = gen(rk)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in mine.items()}
    comm = D._gxd_comm(None)
    res, why = {}, {}

    def op_sort_fused():
        gxd.set_sort_mode(2)        # the exchange between the sort's two partition levels from 2^21 rows per rank
        try:
            out = comm.sort(dev["sort_fused"], force_exchange=True)
            return out.cpu().numpy(), comm.last_timing()[0] == -1.0
        finally:
            gxd.set_sort_mode(0)

    def op_sort_sample():
        return comm.sort(dev["sort_sample"], chunks=2, force_exchange=True).cpu().numpy()

    def op_join():
        hj = gxd.HashJoin(comm, dev["build"], force_exchange=True)
        try:
            l, r = hj.inner_join(dev["probe"], chunks=2)
            return l.cpu().numpy(), r.cpu().numpy()
        finally:
            hj.close()

    def op_groupby():
        k, sm, cnt = comm.groupby_sum_count(dev["gk"], dev["gv"], force_exchange=True)
        return k.cpu().numpy(), sm.cpu().numpy(), cnt.cpu().numpy()

    alive = True
    for name, fn in (("sort_fused", op_sort_fused), ("sort_sample", op_sort_sample), ("join", op_join), ("groupby", op_groupby)):
        if not alive:
            res[name], why[name] = None, "skipped: the communicator was aborted"
            continue
        res[name], why[name] = guarded(c, name, fn, tmo)
        if why[name] and "abort" in why[name]:
            alive = False
    # ---- results to rank 0, oracle there
    gathered = [None] * W if rk == 0 else None
    dist.gather_object({"res": res, "why": why}, gathered, dst=0)
    verdict = {}
    if rk == 0:
        from oracle import c_oracle
        from oracle import cudf_oracle as orc
        ins = [mine if r == 0 else gen(r) for r in range(W)]

        def bases(key):
            b, run = [], 0
            for r in range(W):
                b.append(run)
                run += len(ins[r][key])
            return b
        for name in ("sort_fused", "sort_sample", "join", "groupby"):
            bad = [f"rank {r}: {g['why'][name]}" for r, g in enumerate(gathered) if g["why"][name]]
            if bad:
                verdict[name] = "FAILED to run: " + "; ".join(bad)
                continue
            try:
                if name == "sort_fused":
                    got = np.concatenate([g["res"][name][0] for g in gathered])
                    exp = c_oracle.sort_i64(np.concatenate([i["sort_fused"] for i in ins]))
                    fused = [bool(g["res"][name][1]) for g in gathered]
                    ok = got.tobytes() == exp.tobytes() and (all(fused) or not any(fused))
                    verdict[name] = ("ok (fused path)" if all(fused) else "ok (collective fallback to the sample-sort path)") if ok else "MISMATCH vs oracle"
                elif name == "sort_sample":
                    got = np.concatenate([g["res"][name] for g in gathered])
                    allin = np.concatenate([i["sort_sample"] for i in ins])
                    exp = orc.sort_keys(allin)
                    ok = np.array_equal(got, exp, equal_nan=True) and np.signbit(got[got == 0]).sum() == np.signbit(allin[allin == 0]).sum()
                    verdict[name] = "ok" if ok else "MISMATCH vs oracle"
                elif name == "join":
                    l = np.concatenate([g["res"][name][0] for g in gathered])
                    r_ = np.concatenate([g["res"][name][1] for g in gathered])
                    el, er = c_oracle.inner_join_i64(np.concatenate([i["probe"] for i in ins]), np.concatenate([i["build"] for i in ins]))
                    a = orc.canonical_pairs(l.astype(np.int64), r_.astype(np.int64))
                    b = orc.canonical_pairs(el.astype(np.int64), er.astype(np.int64))
                    ok = len(l) == len(el) and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
                    verdict[name] = f"ok ({len(l)} pairs in global rows)" if ok else f"MISMATCH vs oracle ({len(l)} pairs, oracle {len(el)})"
                else:
                    k = np.concatenate([g["res"][name][0] for g in gathered])
                    sm = np.concatenate([g["res"][name][1] for g in gathered])
                    cn = np.concatenate([g["res"][name][2] for g in gathered])
                    o = np.argsort(k, kind="stable")
                    gk = np.concatenate([i["gk"] for i in ins])
                    gv = np.concatenate([i["gv"] for i in ins])
                    uk = np.unique(gk)
                    es, ec = np.bincount(gk, weights=gv)[uk], np.bincount(gk)[uk]
                    ok = (np.array_equal(k[o], uk) and np.array_equal(cn[o], ec) and np.allclose(sm[o], es, rtol=1e-12, atol=0.0)
                          and len(np.unique(k)) == len(k))
                    verdict[name] = f"ok ({len(k)} groups, every group on one rank)" if ok else "MISMATCH vs oracle"
            except Exception as e:  # noqa: BLE001 -- a checker failure is a failed check
                verdict[name] = f"CHECK RAISED {e!r}"
    box = [verdict]
    dist.broadcast_object_list(box, src=0)
    verdict = box[0]
    verdict["transport"] = "RCCL (ncclAllGather + grouped ncclSend / ncclRecv)" if W > 1 else "one-rank loopback fabric (exchange forced)"
    verdict["ranks"] = W
    verdict["shards"] = "uneven (0.5x / 1x / 1.5x)" + (", rank 1 empty" if W >= 3 else "")
    verdict["seconds"] = round(time.perf_counter() - t_start, 2)
    verdict["communicator_alive"] = alive
    c.beat = time.monotonic()
    return verdict


def sharded_step(c, op, cpp_step, py_step):
    """the step a multi-GPU line times: the C++ operators over RCCL when the pre-flight verified them against the oracle on THIS
    transport; otherwise -- or if their first full-size call raises (decided collectively: every rank takes the same one) -- the
    torch.distributed implementation, and the line says which and why"""
    pf = c.preflight or {}
    names = {"sort": ("sort_fused", "sort_sample"), "join": ("join",), "groupby": ("groupby",)}[op]
    failed = [f"{k}: {pf.get(k)}" for k in names if c.preflight is not None and not str(pf.get(k, "")).startswith("ok")]
    if failed or (c.preflight is not None and not pf.get("communicator_alive", True)):
        return py_step, "torch.distributed fallback (pre-flight of the C++ operator: " + ("; ".join(failed) or "communicator aborted") + ")"
    ok = 1
    try:
        cpp_step()
        c.torch.cuda.synchronize()
    except Exception as e:  # noqa: BLE001
        print(f"bench.py: C++ sharded operator failed on rank {c.rank} ({e!r})", file=sys.stderr)
        ok = 0
    t = c.torch.tensor([ok], device="cuda")
    c.dist.all_reduce(t, op=c.dist.ReduceOp.MIN)
    c.beat = time.monotonic()
    if int(t.item()) == 1:
        return cpp_step, "C++ operators over RCCL" + (", pre-flight checked against the oracle" if c.preflight is not None else "")
    return py_step, "torch.distributed fallback (the C++ operator's first call failed)"


def fetch_by_global_row(c, local_vals, grows, shard_rows):
    """values[g] for global rows g = owner * shard_rows + local row, the values living on their owners: one all-to-all of the
    requests, one of the answers (verification only; equal shard sizes)"""
    from cudf_amd import distributed as D
    torch = c.torch
    W = c.world
    owner = torch.div(grows, shard_rows, rounding_mode="floor")
    order = torch.argsort(owner)
    send = torch.bincount(owner, minlength=W).cpu().tolist()
    recv = D.exchange_counts(send, grows.device) if W > 1 else list(send)
    req_sorted = (grows - owner * shard_rows)[order]
    req = D.all_to_all_rows(req_sorted, send, recv) if W > 1 else req_sorted
    ans = local_vals[req]
    back = D.all_to_all_rows(ans, recv, send) if W > 1 else ans
    out = torch.empty_like(back)
    out[order] = back
    return out


def lsr_mix64(j):
    """splitmix64 finalizer on int64 tensors (a bijection of the 64-bit integers); logical shifts: mask off the sign extension"""
    x = j
    x = (x ^ ((x >> 30) & ((1 << 34) - 1))) * (-4658895280553007687)
    x = (x ^ ((x >> 27) & ((1 << 37) - 1))) * (-7723592293110705685)
    return x ^ ((x >> 31) & ((1 << 33) - 1))


def pmc_traffic(roofline, n):
    """HBM bytes of the step from the COMMITTED PMC passes (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in separate runs of this
    command at 1e9 rows, scripts/gpu_r6.sh <tag> evidence -> profiles/r6_pmc_traffic_1e9.json).  A constant read from a file cannot
    notice a regression in the run it annotates, so it is attached only while it describes THESE kernels: the file records the
    sha256 of the kernel sources it was measured on; when the sources have changed since, `traffic` stays null and
    `traffic_note` says why.  `traffic_source` always names where a figure came from."""
    if roofline is None:
        return
    roofline.setdefault("traffic", None)
    if n != 1_000_000_000:
        roofline["traffic_note"] = "committed PMC passes are for 1e9 rows only"
        return
    key = roofline.get("traffic_key")
    try:
        sys.path.insert(0, os.path.join(ROOT, "scripts"))
        from pmc_to_json import csrc_sha16
        tr = json.load(open(os.path.join(ROOT, "profiles", "r6_pmc_traffic_1e9.json")))
        if tr.get("csrc_sha16") != csrc_sha16():
            roofline["traffic_note"] = ("profiles/r6_pmc_traffic_1e9.json was measured on other kernel sources (sha "
                                        f"{tr.get('csrc_sha16')} != {csrc_sha16()}): not attached")
            return
        e = (tr.get("groups", {}).get(key) or tr["kernels"].get(key)) if key else None
        if e:
            roofline["traffic"] = e["hbm_bytes_per_launch"]
            roofline["traffic_source"] = ("COMMITTED FILE profiles/r6_pmc_traffic_1e9.json, not measured in this run: " + tr["source"] + "; " +
                                          tr["correction"] + (f"; sum over {e['members']}" if "members" in e else ""))
        else:
            roofline["traffic_note"] = f"no entry {key!r} in profiles/r6_pmc_traffic_1e9.json"
    except (OSError, KeyError, ValueError, ImportError) as ex:
        roofline["traffic_note"] = f"no committed PMC file for this build ({type(ex).__name__})"


DUMP_ROWS = 1 << 21   # rows per --dump-outputs file: int64 keys make two files of 16 MB, inside the 64-MB budget


def dump_rows(n, m=DUMP_ROWS, seed=2026):
    """the rows --dump-outputs writes: all n up to m, else one seeded position in each of m equal ranges (ascending, the same every run)"""
    import numpy as np
    if n <= m:
        return np.arange(n, dtype=np.int64)
    edges = np.arange(m + 1, dtype=np.int64) * n // m
    return edges[:-1] + np.random.default_rng(seed).integers(0, edges[1:] - edges[:-1])


def dump_outputs(c, col, dt):
    """--dump-outputs: the column the timed path returned (dtype dt), at the rows of dump_rows(), as float64 .npy files; int64
    values are split into two exact halves, since float64 holds 53 bits"""
    np = c.np
    t = c.as_tensor(col, dt)
    v = t[c.torch.from_numpy(dump_rows(col.size)).to(t.device)].cpu().numpy()
    if dt == c.torch.int64:
        files = {"sorted_keys_hi32": v >> 32, "sorted_keys_lo32": v & 0xFFFFFFFF}
    else:
        files = {"sorted_order" if dt == c.torch.int32 else "sorted_keys": v}
    os.makedirs(c.args.dump_outputs, exist_ok=True)
    for name, a in files.items():
        np.save(os.path.join(c.args.dump_outputs, name + ".npy"), a.astype(np.float64))


# ------------------------------------------------------------------------------------------------
# config 2: radix sort
# ------------------------------------------------------------------------------------------------

def bench_sort(c, pairs=False, cpu_leg=True, dump=False):
    a, lib, L, ops, np = c.args, c.lib, c.L, c.ops, c.np
    n = c.n
    lib.gx_sort_set_algorithm(a.algo)
    lib.gx_sort_set_hybrid(0 if a.no_hybrid else 1)
    lib.gx_sort_set_cell(a.sort_cell)
    lib.gx_sort_set_lookback(a.sort_lbw)
    lib.gx_sort_set_cursor_path(0 if a.no_cursor else 1, 0.0)
    lib.gx_sort_set_splitters(a.sort_splitters)
    if a.key_range:
        keys = ops.random_column(np.int64, n, seed=42 + c.rank, lo=a.key_range[0], hi=a.key_range[1])
    else:
        keys = ops.random_column(np.int64, n, seed=42 + c.rank)
    is_f64 = getattr(a, "key_type", "int64") == "float64"
    if is_f64:
        # a FLOAT64 column of ordinary data: N(0, 1) (default) or U[0, 1) doubles -- no NaN, no -0.0
        torch = c.torch
        keys = c.Column.empty(np.float64, n)
        ft = c.as_tensor(keys, torch.float64)
        g = torch.Generator(device="cuda").manual_seed(42 + c.rank)
        step = 1 << 27
        for i in range(0, n, step):
            m = min(step, n - i)
            if a.key_dist == "uniform":
                ft[i:i + m] = torch.rand(m, generator=g, device="cuda", dtype=torch.float64)
            else:
                ft[i:i + m] = torch.randn(m, generator=g, device="cuda", dtype=torch.float64)
        ft[ft == 0] = 1.0
        del ft
        torch.cuda.synchronize()
    elif a.key_dist != "uniform":
        torch = c.torch
        kt = c.as_tensor(keys, torch.int64)
        if a.key_dist == "sorted":
            kt.copy_(torch.sort(kt).values)
        elif a.key_dist == "dupids":
            del kt
            keys = ops.random_column(np.int64, n, seed=42 + c.rank, lo=0, hi=max(1, n // max(1, a.key_copies)))
            kt = c.as_tensor(keys, torch.int64)
            kt.mul_(-7046029254386353131)   # x * 0x9E3779B97F4A7C15 mod 2^64: distinct ids spread over the 64-bit range
        else:
            g = torch.Generator(device="cuda").manual_seed(42 + c.rank)
            step = 1 << 27
            for i in range(0, n, step):           # in pieces: the float64 temporaries stay at 1 GB
                m = min(step, n - i)
                if a.key_dist == "normal":
                    kt[i:i + m] = (torch.randn(m, generator=g, device="cuda", dtype=torch.float64) * float(1 << 40)).round_().to(torch.int64)
                elif a.key_dist == "lognormal":   # round(exp(N(25, 3))): densities over many octaves
                    kt[i:i + m] = torch.randn(m, generator=g, device="cuda", dtype=torch.float64).mul_(3.0).add_(25.0).exp_().round_().clamp_(max=9.0e18).to(torch.int64)
                elif a.key_dist == "clusters":    # two far-apart clusters: -2^50 + N(0, 2^30) and 2^50 + N(0, 2^30)
                    side = torch.rand(m, generator=g, device="cuda", dtype=torch.float64) < 0.5
                    kt[i:i + m] = (torch.randn(m, generator=g, device="cuda", dtype=torch.float64) * float(1 << 30)).round_().to(torch.int64) + torch.where(side, -(1 << 50), 1 << 50)
                else:
                    u = torch.rand(m, generator=g, device="cuda", dtype=torch.float64).clamp_(min=2.0 ** -53)
                    kt[i:i + m] = u.pow_(-5.0).clamp_(max=float(1 << 31)).floor_().to(torch.int64)
        del kt
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    if a.hot_copies:
        # a HOT VALUE: `hot_copies` rows (every (n // hot_copies)-th, so every input range holds its share) carry one key -- the
        # zeros / sentinel / default-id case that used to send the whole column to the LSD passes (VERDICT r3 "missing" 2)
        kt = c.as_tensor(keys, c.torch.int64)
        kt[:: max(1, n // int(a.hot_copies))] = 1234567890123
        del kt
    out = c.Column.empty(np.int32 if pairs else (np.float64 if is_f64 else np.int64), n)
    nb = ctypes.c_size_t(0)
    if pairs:
        fn = lambda tmp, nbp: lib.gx_sorted_order(keys.gx, keys.data_ptr, None, n, 0, 0, 1, out.data_ptr, tmp, nbp, c.stream)
    else:
        fn = lambda tmp, nbp: lib.gx_sort_keys(keys.gx, keys.data_ptr, out.data_ptr, n, 0, tmp, nbp, c.stream)
    L.check(fn(None, ctypes.byref(nb)), "size query")
    tmp = c.device_bytes(nb.value)
    single_step = lambda: L.check(fn(c.ptr(tmp), ctypes.byref(nb)), "sort")
    # round 6: sorted_order of a 64-bit column from 2^25 rows = a keys-only sort of (monotone rank << row bits | row) words + a pass
    # that puts runs of equal ranks right (cudf_amd/csrc/gx_order.hip): its partition / cell kernels move keys-only 16 B/row
    lib.gx_sort_set_order_map(getattr(a, "sort_order_map", 1))
    order_map = bool(pairs and lib.gx_order_map_applies(keys.gx, n))
    bytes_per_row_pass = 24 if (pairs and not order_map) else 16   # read key(+idx) + write key(+idx)
    model_bytes_row = 200 if pairs else 136    # 8-pass LSD model
    workload = f"{n:.0e}-row " + ("float64 " if is_f64 else "int64 ") + (("sorted_order (keys-only sort of (rank, row) words + run fix-up, int32 order out)" if order_map else
                                                                          "sorted_order (radix sort pairs, int32 payload)") if pairs else "radix sort (cudf::sort, keys only)")
    if is_f64:
        workload += ", keys " + ("U[0, 1)" if a.key_dist == "uniform" else "N(0, 1)")
    if a.key_range:
        workload += f", keys uniform in [{a.key_range[0]}, {a.key_range[1]})"
    if a.hot_copies:
        workload += f", {int(a.hot_copies):.0e} copies of one value"
    if a.key_dist != "uniform" and not is_f64:
        workload += f", {a.key_dist} keys" + (f" ({a.key_copies} rows per id)" if a.key_dist == "dupids" else "")

    prof = {"pass_ms": 0.0, "hist_ms": 0.0, "launches": 0, "hyb": [0.0] * 4, "hyb_n": 0}

    def read_profile():
        # reading the events waits for this step only; it is part of the timed region
        h = ctypes.c_float()
        p = (ctypes.c_float * 8)()
        k = ctypes.c_int()
        L.check(lib.gx_sort_profile_read(ctypes.byref(h), p, ctypes.byref(k)), "profile_read")
        act = [x for x in list(p)[: k.value] if x > 0.05]  # skipped passes exit in microseconds
        prof["pass_ms"] += sum(act)
        prof["launches"] += len(act)
        prof["hist_ms"] += h.value
        h4 = (ctypes.c_float * 4)()
        if lib.gx_sort_profile_read_hybrid(h4) == 0:
            for i in range(4):
                prof["hyb"][i] += h4[i]
            prof["hyb_n"] += 1

    if c.sharded:
        from cudf_amd import distributed as D
        dkeys = c.as_tensor(keys, c.torch.int64)
        # CUDA tensors and no `local` object: the C++ operators over RCCL (cudf_amd/cpp/src/distributed.cpp, gxd_sort), which the
        # pre-flight has just checked against the oracle on this very transport; where it failed, or should the first full-size
        # call raise, the torch.distributed implementation of round 2 takes over and the line says so.
        step, sharded_impl = sharded_step(c, "sort", lambda: D.distributed_sort(dkeys), lambda: D.distributed_sort(dkeys, local=D.HipLocalOps()))
        workload = (f"{n:.0e}-row-per-GPU int64 distributed sort (level 0 on every rank, level-0 bins dealt to ranks, one span per peer over "
                    f"xGMI, level 1 + cell sort on the receiver) [{sharded_impl}]")
        sec = c.timed(step)
        res = step()
        torch = c.torch
        assert bool((res[1:] >= res[:-1]).all()), "distributed sort: shard not sorted"
        tot = c.torch.tensor([res.numel()], device="cuda", dtype=c.torch.int64)
        c.dist.all_reduce(tot)
        assert int(tot.item()) == n * c.world, "distributed sort lost rows"
        # shard r's largest key <= shard r + 1's smallest (empty shards carry neutral bounds)
        big = torch.iinfo(torch.int64)
        mm = torch.tensor([int(res[0].item()) if res.numel() else big.max, int(res[-1].item()) if res.numel() else big.min], device="cuda", dtype=torch.int64)
        allmm = [torch.zeros_like(mm) for _ in range(c.world)]
        c.dist.all_gather(allmm, mm)
        hi = big.min
        for t in allmm:
            lo_r, hi_r = int(t[0].item()), int(t[1].item())
            if lo_r <= hi_r:
                assert lo_r >= hi, "distributed sort: shards overlap"
                hi = hi_r
        checked = "every rank's shard sorted; shard boundaries ordered over the ranks; row count over all ranks; see `preflight` for the oracle check of the same operators"
        del res
        # roofline of the dominant LOCAL kernel: one profiled single-GPU sort of this rank's shard, untimed
        lib.gx_sort_profile(1)
        single_step()
        read_profile()
        nsteps_prof = 1
    else:
        if a.full:
            # the timed steps carry the two events around the FIRST partition level only (gx_sort_profile(2)): an event between two kernels
            # costs the stream ~15 us and the full set is 23 per sort -- 0.35 ms of an 11-ms step that no caller of cudf::sort pays.  The
            # other kernels' durations come from ONE more call with every event, outside the timed region (`kernels_ms_note`).
            sec = c.timed(single_step, after_warmup=lambda: lib.gx_sort_profile(2), slot=lib.gx_sort_profile_slot, read_slot=read_profile)
        else:
            sec = c.timed(single_step)   # a plain run: no event inside the timed steps, they serve the roofline of --full only
        if dump:
            dump_outputs(c, out, c.torch.int32 if pairs else (c.torch.float64 if is_f64 else c.torch.int64))
        if not a.full:
            st = ctypes.c_int(0)
            lib.gx_sort_status(c.ptr(tmp), ctypes.byref(st), c.stream)
            assert st.value == 0, "look-back timed out"
            return {"workload": workload, "rows": n, "ms_per_step": sec * 1e3, "rows_per_s": n * c.world / sec, "dtype": "f64" if is_f64 else "int64",
                    "roofline": None, "cpu_baseline": None, "checked": None}
        nsteps_prof = a.steps
        live_l0 = prof["hyb"][0] / prof["hyb_n"] if prof["hyb_n"] else None
        prof.update({"pass_ms": 0.0, "hist_ms": 0.0, "launches": 0, "hyb": [0.0] * 4, "hyb_n": 0})
        lib.gx_sort_profile(1)
        single_step()
        read_profile()
        nsteps_prof = 1
        if live_l0 is not None and prof["hyb_n"]:
            prof["hyb"][0] = live_l0   # (hyb_n == 1: the three other intervals are this call's)
            prof["live_level0"] = True
        cin = ops.checksum(keys)
        if not pairs:
            cout = ops.checksum(out)
            assert cout[2] == 0 and cin[:2] == cout[:2], "sort output invalid"
            checked = "order + multiset checksum of the timed output (gx_checksum)"
        else:
            # cudf::sorted_order's timed output, checked at full size: (1) the int32 order is a PERMUTATION of
            # [0, n) -- every row marked exactly once; (2) the keys gathered through it are in order and are the input's multiset
            # (gx_checksum: sum, xor, sortedness violations); (3) ties keep the row order (stable: sorted_order_radix.cu:56-179)
            torch = c.torch
            ot = c.as_tensor(out, torch.int32)
            assert int(ot.min().item()) >= 0 and int(ot.max().item()) < n, "sorted_order: row index out of range"
            seen = torch.zeros(n, dtype=torch.int32, device="cuda")
            CH = 1 << 27
            for i in range(0, n, CH):
                seen.index_add_(0, ot[i:i + CH].to(torch.int64), torch.ones(min(CH, n - i), dtype=torch.int32, device="cuda"))
            assert int(seen.min().item()) == 1 and int(seen.max().item()) == 1, "sorted_order: the output is not a permutation of the rows"
            del seen
            gathered = ops.gather(keys, out)
            cg = ops.checksum(gathered)
            assert cg[2] == 0 and cin[:2] == cg[:2], "sorted_order: keys gathered through the order are not the sorted input"
            gt = c.as_tensor(gathered, torch.int64)   # (float64 keys of the bench hold no NaN and no zero: equal bits == equal values)
            for i in range(0, n - 1, CH):
                m = min(CH, n - 1 - i)
                eq = gt[i + 1:i + 1 + m] == gt[i:i + m]
                assert bool((ot[i + 1:i + 1 + m][eq] > ot[i:i + m][eq]).all()), "sorted_order: equal keys are not in row order"
            del gathered, gt, ot
            torch.cuda.empty_cache()
            checked = ("timed int32 order at full size: a permutation of [0, n); keys gathered through it: order + multiset checksum "
                       "(gx_checksum) equal to the input's; equal keys in ascending row order")
        st = ctypes.c_int(0)
        lib.gx_sort_status(c.ptr(tmp), ctypes.byref(st), c.stream)
        assert st.value == 0, "look-back timed out"
    lib.gx_sort_profile(0)
    ms_per_step = sec * 1e3
    info = (ctypes.c_int32 * 8)()
    lib.gx_sort_info(c.ptr(tmp), info, c.stream)
    sort_info = dict(zip(["hybrid_attempted", "hybrid_used", "shift0", "shift2", "bits2", "lds_passes", "max_cell", "lsd_passes"], list(info)))
    cst = ctypes.c_int32(0)
    lib.gx_sort_cursor_state(c.ptr(tmp), ctypes.byref(cst), c.stream)
    sort_info["cursor_path_state"] = cst.value  # 3: sample-planned, atomic-cursor partition levels; 0 / 2: look-back path
    bigi = (ctypes.c_int64 * 3)()
    lib.gx_sort_big_info(c.ptr(tmp), bigi, c.stream)
    sort_info["big_cells"] = {"sorted_through_x": int(bigi[0]), "cells": int(bigi[1]), "keys": int(bigi[2])}
    spi = (ctypes.c_int32 * 4)()
    lib.gx_sort_split_info(c.ptr(tmp), spi, c.stream)
    sort_info["splitters"] = {"on": int(spi[0]), "splitters": int(spi[1]), "equality_buckets": int(spi[2])}
    cursor = cst.value == 3
    hist_ms = prof["hist_ms"] / nsteps_prof
    local_sort_ms = ms_per_step if not c.sharded else hist_ms + (sum(prof["hyb"]) if prof["hyb_n"] else prof["pass_ms"])
    roofline = None
    if sort_info["hybrid_used"] and prof["hyb_n"]:
        # hybrid MSD path: per-kernel algorithmic bytes: partition passes and the local sort read 8 +
        # write 8 B/row, the joint histogram reads 8 B/row
        ms = [x / prof["hyb_n"] for x in prof["hyb"]]
        todo = ctypes.c_int32(-1)
        lib.gx_sort_place_info(c.ptr(tmp), ctypes.byref(todo), c.stream)
        sort_info["cells"] = 256 << sort_info["bits2"]
        sort_info["cells_left_to_k_local_sort"] = todo.value  # crowded cells of k_local_place (a 13-bit bin with > 9 keys)
        names = ["k_msd_pass level 0 (8-bit partition, 8 XCD chains)",
                 f"k_msd_pass level 1 ({sort_info['bits2']}-bit partition inside buckets, padded cell slots)",
                 "k_plan2 (cell starts, one block)",
                 "k_local_place + k_local_sort (LDS sort of the cells: counting placement + per-thread window networks; crowded cells: sub-bucket path)"
                 if sort_info["max_cell"] <= 8192 else "k_local_sort (LDS sort of the cells)"]
        tkeys = ["k_msd_pass level 0", "k_msd_pass level 1", "k_plan2", "sort local stage"]
        if cursor:
            names[0] = "k_hf_scatter level 0 (8-bit partition into sampled (range, bin) slots, cursor atomics) + verdict"
            names[1] = f"k_hf_scatter level 1 ({sort_info['bits2']}-bit partition of the regions into padded cell slots, cursor atomics)"
            tkeys[0], tkeys[1] = "k_hf_scatter level 0", "k_hf_scatter level 1"
        up_front = 0 if cursor else 8  # B/row of the up-front pass: the cursor path reads a 1/32 sample instead of the column
        bpr = [20, 24, 0, 24] if (pairs and not order_map) else [16, 16, 0, 16]  # pairs carry a 4-B index (the word sort of round 6 moves 8-byte words)
        if order_map:
            up_front = 16 + 12  # the map pass (8 B key in, 8 B word out) and the finish pass (8 B word in, 4 B row out) around the word sort
        # the kernel priced: the first partition level where it was measured inside the timed steps (the three big kernels are within
        # ~8 % of each other; rocprofv3 has level 0 at or near the top), else the longest interval of the profiled call
        dom = 0 if prof.get("live_level0") else max(range(4), key=lambda i: ms[i])
        achieved = bpr[dom] * n / (ms[dom] * 1e-3) / 1e9
        roofline = {"bound": "hbm", "kernel": names[dom], "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": achieved / HBM_PEAK_GBS, "traffic": None, "traffic_key": tkeys[dom], "algorithmic_bytes_per_launch": bpr[dom] * n,
                    "avg_launch_ms": ms[dom], "launches_per_step": 1.0,
                    "kernels_ms": dict(zip(names, ms)), "kernels_GBps": {k: b * n / (m * 1e-3) / 1e9 for k, b, m in zip(names, bpr, ms) if b},
                    "hist_kernel_ms": hist_ms,
                    "kernels_ms_note": ("first entry: HIP events around that launch inside each of the K timed steps, averaged; the other entries: "
                                        "one more call with every event recorded, outside the timed region") if prof.get("live_level0") else
                                       "HIP events of one profiled call",
                    "path_bytes_per_row": up_front + sum(bpr), "path_GBps": (up_front + sum(bpr)) * n / (local_sort_ms * 1e-3) / 1e9,
                    "path_frac": (up_front + sum(bpr)) * n / (local_sort_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                    "whole_sort_model_GBps": model_bytes_row * n / (local_sort_ms * 1e-3) / 1e9,
                    "whole_sort_model_frac": model_bytes_row * n / (local_sort_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                    "sort_info": sort_info}
        if order_map:
            omi = (ctypes.c_int32 * 5)()
            lib.gx_sort_order_map_info(c.ptr(tmp), n, omi, c.stream)
            roofline["order_map"] = {"long_runs": int(omi[0]), "row_bits": int(omi[2]), "rank_bits_in_bucket": int(omi[3]), "inexact_buckets": int(omi[4]),
                                     "note": "the kernels above are those of the WORD sort (gx_sort_keys on uint64 words); map + finish = total - their sum"}
    elif prof["launches"]:
        avg_ms = prof["pass_ms"] / prof["launches"]
        achieved = bytes_per_row_pass * n / (avg_ms * 1e-3) / 1e9
        roofline = {"bound": "hbm", "kernel": "k_radix_pass (one 8-bit digit scatter pass)", "achieved": achieved,
                    "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": None,
                    "algorithmic_bytes_per_launch": bytes_per_row_pass * n, "avg_launch_ms": avg_ms,
                    "launches_per_step": prof["launches"] / nsteps_prof, "hist_kernel_ms": hist_ms,
                    "whole_sort_model_GBps": model_bytes_row * n / (local_sort_ms * 1e-3) / 1e9,
                    "whole_sort_model_frac": model_bytes_row * n / (local_sort_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                    "sort_info": sort_info}
    pmc_traffic(roofline, n)
    cpu = None
    if a.cpu and cpu_leg and not c.sharded and c.rank == 0:
        cpu = cpu_baseline_sort(a.cpu_rows or 5e8, a.cpu_rows_pandas or 1e8)
    return {"workload": workload, "rows": n, "ms_per_step": ms_per_step, "rows_per_s": n * c.world / sec, "dtype": "f64" if is_f64 else "int64",
            "roofline": roofline, "cpu_baseline": cpu, "checked": checked}


# ------------------------------------------------------------------------------------------------
# config 3: inner hash join, probe 1e9 x build 1e8, selectivity 0.3
# ------------------------------------------------------------------------------------------------

def bench_join(c):
    a, lib, L, ops, np, torch = c.args, c.lib, c.L, c.ops, c.np, c.torch
    n = c.n
    nb_rows = max(1, n // 10)
    lib.gx_join_set_probe_kernel(a.join_probe_kernel)
    lib.gx_join_set_scatter_tile(a.join_scatter_tile)
    lib.gx_join_set_experiment(a.join_xp)
    lib.gx_join_set_build_kernel(a.join_build_kernel)
    if c.sharded:
        from cudf_amd import distributed as D
        W, rk = c.world, c.rank
        if a.rows == 1e9 and W > 1:
            n = 1_250_000_000        # BASELINE config 5: 1e10 probe rows over 8 GPUs = 1.25e9 per GPU (weak scaling: the same at every N > 1)
            nb_rows = n // 10
        # SURVEY 8d's key distribution, as on one GPU (no arithmetic progressions): build = random DISTINCT 64-bit
        # keys, mix64(j + (rank << 40)) with j a random permutation of [0, nb_rows) -- a bijection, so distinct over all ranks;
        # probe = 30 % hits drawn uniformly from the build keys of ALL ranks, 70 % from the disjoint set j >= nb_rows
        torch.manual_seed(12345 + rk)
        dbk = lsr_mix64(torch.randperm(nb_rows, device="cuda") + (rk << 40))
        dpk = torch.empty(n, dtype=torch.int64, device="cuda")
        hit_mask = torch.empty(n, dtype=torch.bool, device="cuda")
        CH = 1 << 27
        for s0 in range(0, n, CH):   # in pieces: a few 1-GB temporaries instead of 10-GB ones
            m = min(CH, n - s0)
            selt = c.as_tensor(ops.random_column(np.int64, m, seed=67890 + 131 * rk + (s0 >> 27), lo=0, hi=10), torch.int64)
            jj = c.as_tensor(ops.random_column(np.int64, m, seed=424242 + 131 * rk + (s0 >> 27), lo=0, hi=nb_rows), torch.int64)
            src = c.as_tensor(ops.random_column(np.int64, m, seed=515151 + 131 * rk + (s0 >> 27), lo=0, hi=W), torch.int64)
            hit_mask[s0:s0 + m] = selt < 3
            dpk[s0:s0 + m] = lsr_mix64(jj + (selt >= 3).to(torch.int64) * nb_rows + (src << 40))
            del selt, jj, src
        # like the single-GPU line (and cudf::hash_join): the build side is exchanged and hashed ONCE, untimed;
        # a step = hash-partition the probe shard, all-to-all, probe the local table
        use_cpp = c.preflight is None or (str(c.preflight.get("join", "")).startswith("ok") and c.preflight.get("communicator_alive", True))
        tb = time.perf_counter()
        impl = "C++ operators over RCCL" + (", pre-flight checked against the oracle" if c.preflight is not None else "")
        hj, ok = None, 1
        if use_cpp:
            try:
                hj = D.DistributedHashJoin(dbk)         # gxd_join_build / gxd_join_probe
                hj.inner_join(dpk[: 1 << 20])
                torch.cuda.synchronize()
            except Exception as e:  # noqa: BLE001 -- decided collectively below
                print(f"bench.py: C++ sharded join failed on rank {rk} ({e!r})", file=sys.stderr)
                ok = 0
            t = torch.tensor([ok], device="cuda")
            c.dist.all_reduce(t, op=c.dist.ReduceOp.MIN)
            ok = int(t.item())
        if not use_cpp or not ok:
            impl = "torch.distributed fallback (" + ("pre-flight of the C++ operator: " + str((c.preflight or {}).get("join")) if not use_cpp
                                                    else "the C++ operator's first call failed") + ")"
            hj = D.DistributedHashJoin(dbk, local=D.HipLocalOps())
        torch.cuda.synchronize()
        c.beat = time.monotonic()
        build_ms = (time.perf_counter() - tb) * 1e3
        step = lambda: hj.inner_join(dpk)
        sec = c.timed(step)
        l, r = step()
        # ---- guards on the (re-run) timed step: pair count = closed form; the probe rows that appear are exactly the hit rows of
        # all ranks (sum and sum of squares of the global rows, wrapping); EVERY pair joins equal keys -- the probe key at the
        # pair's global probe row and the build key at its global build row are fetched from their owners and compared
        tot = torch.tensor([l.numel()], device="cuda", dtype=torch.int64)
        c.dist.all_reduce(tot)
        want = hit_mask.sum().to(torch.int64).reshape(1)
        c.dist.all_reduce(want)
        assert int(tot.item()) == int(want.item()), f"distributed join: {int(tot.item())} pairs, closed form {int(want.item())}"
        rows = torch.nonzero(hit_mask).flatten() + rk * n
        sums = torch.stack([l.sum(), (l * l).sum(), rows.sum(), (rows * rows).sum()])
        c.dist.all_reduce(sums)
        assert int(sums[0].item()) == int(sums[2].item()) and int(sums[1].item()) == int(sums[3].item()), "distributed join: wrong set of probe rows"
        del rows
        checked = "pair count == closed form over all ranks; the global probe rows are exactly the hit rows (sum, sum of squares)"
        try:
            pkeys = fetch_by_global_row(c, dpk, l, n)
            bkeys = fetch_by_global_row(c, dbk, r, nb_rows)
            eq = torch.tensor([int((pkeys == bkeys).all().item())], device="cuda")
            c.dist.all_reduce(eq, op=c.dist.ReduceOp.MIN)
            assert int(eq.item()) == 1, "distributed join: a pair joins unequal keys"
            checked += "; every pair joins equal keys (keys fetched from the owners of its global rows)"
            del pkeys, bkeys
        except AssertionError:
            raise
        except Exception as e:  # noqa: BLE001 -- the verification exchange itself failed: say so, keep the checks that ran
            checked += f"; key equality per pair NOT checked ({e!r})"
        c.beat = time.monotonic()
        return {"workload": f"{n:.3g}-row-per-GPU probe x {nb_rows:.3g}-row-per-GPU build distributed inner join, random distinct 64-bit build keys, "
                            f"probe 30 % hits over all ranks' keys (build side exchanged and hashed once; step = hash partition of the probe shard, "
                            f"all-to-all, local probe) [{impl}]",
                "rows": n, "ms_per_step": sec * 1e3, "rows_per_s": n * c.world / sec, "dtype": "int64", "roofline": None,
                "cpu_baseline": None, "build_ms": build_ms, "partition_bits": None, "matches": int(tot.item()), "join_keys": "random",
                "checked": checked}
    lib.gx_join_set_partition_mode(a.join_spec, a.join_early_loads)
    bk = c.Column.empty(np.int64, nb_rows)
    bkt = c.as_tensor(bk, torch.int64)
    torch.manual_seed(12345 + c.rank)
    if a.join_keys == "dense":
        # round 2's keys: arithmetic progressions -- under the table's multiplicative slot hash a low-discrepancy sequence
        # (near-zero collisions, perfectly even partitions); kept only to show what that flattered
        bkt.copy_(torch.randperm(nb_rows, device="cuda") * 3 + 1)  # distinct keys {3i+1}, shuffled
        pk = ops.random_column(np.int64, n, seed=67890 + c.rank, lo=0, hi=int(nb_rows / 0.3))
        pkt = c.as_tensor(pk, torch.int64)
        pkt.mul_(3).add_(1)                                        # hits a build key w.p. 0.3
        is_hit = lambda: pkt < (3 * nb_rows + 1)
    else:
        # SURVEY 8d / cpp/benchmarks/join/generate_input_tables.cu:24-103: build = a random permutation of a random SET of
        # distinct 64-bit keys, probe = selectivity 0.3 drawn uniformly from the build keys, the rest from a disjoint
        # random set of equal size.  The set is mix64(j), j in [0, 2 * nb_rows): mix64 (the splitmix64 finalizer) is a
        # bijection of the 64-bit integers, so the values are distinct and look random in every bit; j < nb_rows is the
        # build set, j >= nb_rows the disjoint one.

        bkt.copy_(lsr_mix64(torch.randperm(nb_rows, device="cuda") + (c.rank << 40)))
        pk = c.Column.empty(np.int64, n)
        pkt = c.as_tensor(pk, torch.int64)
        sel = ops.random_column(np.int64, n, seed=67890 + c.rank, lo=0, hi=10)            # < 3: a hit
        jj = c.as_tensor(ops.random_column(np.int64, n, seed=424242 + c.rank, lo=0, hi=nb_rows), torch.int64)
        selt = c.as_tensor(sel, torch.int64)
        jj.add_((selt >= 3).to(torch.int64) * nb_rows).add_(c.rank << 40)
        hit_mask = selt < 3
        CH = 1 << 27
        for s0 in range(0, n, CH):   # in chunks: the mix needs a few temporaries
            pkt[s0:s0 + CH] = lsr_mix64(jj[s0:s0 + CH])
        del jj, sel, selt
        is_hit = lambda: hit_mask
    hj = ops.HashJoin(bk)  # warm-up build (allocations, module load)
    torch.cuda.synchronize()
    tb = time.perf_counter()
    hj = ops.HashJoin(bk)
    torch.cuda.synchronize()
    build_call_ms = (time.perf_counter() - tb) * 1e3  # one cudf::hash_join construction as a caller sees it (host clock, allocations included)
    # the build itself, like the probe below: scratch allocated once, K builds into the same table between HIP events
    # (the reference's join benchmark times build + probe together: cpp/benchmarks/join/join_common.hpp:83-122)
    build_ms = build_call_ms
    if lib.gx_join_partition_bits(8, hj.table_bytes) > 0 and nb_rows >= (1 << 20):
        bnb = ctypes.c_size_t(0)
        L.check(lib.gx_join_build_partitioned(8, bk.data_ptr, nb_rows, c.ptr(hj.table), hj.table_bytes, 0.5, None, ctypes.byref(bnb), c.stream), "query")
        btmp = c.device_bytes(bnb.value)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        reps = max(3, a.steps)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            L.check(lib.gx_join_build_partitioned(8, bk.data_ptr, nb_rows, c.ptr(hj.table), hj.table_bytes, 0.5, c.ptr(btmp), ctypes.byref(bnb), c.stream), "build")
        e1.record()
        torch.cuda.synchronize()
        build_ms = e0.elapsed_time(e1) / reps
        del btmp
    lo = c.Column.empty(np.int32, n)
    ro = c.Column.empty(np.int32, n)
    cur = torch.zeros(1, dtype=torch.int64, device="cuda")
    part_bits = lib.gx_join_partition_bits(8, hj.table_bytes) if not a.no_partitioned_join else 0
    jnb = ctypes.c_size_t(0)
    if part_bits:
        L.check(lib.gx_join_probe_partitioned(8, pk.data_ptr, n, c.ptr(hj.table), hj.table_bytes, 0, lo.data_ptr,
                                              ro.data_ptr, n, c.ptr(cur), None, ctypes.byref(jnb), c.stream), "query")
        jtmp = c.device_bytes(jnb.value)

    def step():
        cur.zero_()
        if part_bits:
            L.check(lib.gx_join_probe_partitioned(8, pk.data_ptr, n, c.ptr(hj.table), hj.table_bytes, 0, lo.data_ptr,
                                                  ro.data_ptr, n, c.ptr(cur), c.ptr(jtmp), ctypes.byref(jnb), c.stream), "probe")
        else:
            L.check(lib.gx_join_probe(8, pk.data_ptr, None, n, c.ptr(hj.table), hj.table_bytes, 0, lo.data_ptr,
                                      ro.data_ptr, n, c.ptr(cur), c.stream), "probe")

    kms = [0.0, 0.0, 0.0]
    kn = [0]

    def read_profile():
        ms3 = (ctypes.c_float * 3)()
        if part_bits and lib.gx_join_profile_read(ms3) == 0:
            for i in range(3):
                kms[i] += ms3[i]
            kn[0] += 1

    sec = c.timed(step, after_warmup=lambda: lib.gx_join_profile(1), slot=lib.gx_join_profile_slot, read_slot=read_profile)
    lib.gx_join_profile(0)
    ms_per_step = sec * 1e3
    # ---- guard on the timed output: the number of pairs is the closed form, every pair joins equal keys, and
    # the probe rows that appear are exactly the matching rows (sum and sum of squares of their indices)
    matches = int(cur.item())
    if not a.join_unchecked:
        hit = is_hit()
        want = int(hit.sum().item())
        assert matches == want, f"join: {matches} pairs, closed form {want}"
        lt = c.as_tensor(lo, torch.int32)[:matches].to(torch.int64)
        rt = c.as_tensor(ro, torch.int32)[:matches].to(torch.int64)
        assert bool((pkt[lt] == bkt[rt]).all()), "join: a pair joins unequal keys"
        rows = torch.nonzero(hit).flatten()
        assert int(lt.sum().item()) == int(rows.sum().item()), "join: wrong set of probe rows (sum)"
        assert int((lt * lt).sum().item()) == int((rows * rows).sum().item()), "join: wrong set of probe rows (sum of squares)"
        del lt, rt, rows, hit
    algb = 24 * n + 16 * matches   # 24 B/probe row + 16 B/match
    ach = algb / (ms_per_step * 1e-3) / 1e9
    spec = bool(a.join_spec)
    roofline = {"bound": "hbm",
                "kernel": ("k_probe" if not part_bits else
                           ("partitioned probe (k_pj2_scatter + k_pj2_offsets + " + ("k_pj3_probe_direct" if a.join_probe_kernel in (2, 3) else "k_pj2_probe_pipe") +
                            ": hist-free speculative partition)") if spec else
                           "partitioned probe (k_pj_hist + k_pj_scatter + k_pj_probe_pipe)"),
                "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS, "traffic": None,
                "traffic_key": None if not part_bits else ("join probe phase" if spec else "join probe phase (exact two-pass)"),
                "algorithmic_bytes_per_launch": algb, "avg_launch_ms": ms_per_step, "matches": matches,
                "model": "24 B/probe row + 16 B/match (SURVEY.md 8d); whole probe phase = " + ("2 launches + a region-table kernel" if spec else "3 launches")}
    if kn[0]:
        ms = [x / kn[0] for x in kms]
        names = ["k_pj_hist+k_pj_offsets (partition histogram; a no-op on the speculative path)",
                 ("k_pj2_scatter" if spec else "k_pj_scatter") + " (partition (key,row) by table hash)",
                 (("k_pj3_probe_direct (direct probe of L2-resident sub-tables, no tags)" if a.join_probe_kernel in (2, 3) else
                   "k_pj2_probe_pipe (tag probe of partition-resident sub-tables)") if spec else "k_pj_probe_pipe (tag probe of partition-resident sub-tables)")]
        kb = [8 * n, 20 * n, 12 * n + 8 * matches]   # bytes each launch must move: keys | keys + (key,row) | (key,row) + pairs
        dom = max(range(3), key=lambda i: ms[i])
        roofline["kernels_ms"] = dict(zip(names, ms))
        roofline["kernels_GBps"] = {k: b / (m * 1e-3) / 1e9 for k, b, m in zip(names, kb, ms)}
        roofline["dominant_kernel"] = {"kernel": names[dom], "algorithmic_bytes_per_launch": kb[dom], "avg_launch_ms": ms[dom],
                                       "achieved": kb[dom] / (ms[dom] * 1e-3) / 1e9,
                                       "frac": kb[dom] / (ms[dom] * 1e-3) / 1e9 / HBM_PEAK_GBS}
        roofline["path_bytes"] = sum(kb)
        roofline["path_GBps"] = sum(kb) / (ms_per_step * 1e-3) / 1e9
    pmc_traffic(roofline, n)
    cpu = None
    if a.cpu and c.rank == 0:
        cpu = cpu_baseline_join(a.cpu_rows or 1e8, a.cpu_rows_pandas or 1e7)
    keydesc = ("random distinct 64-bit build keys, probe 30 % from them + 70 % from a disjoint random set (SURVEY 8d)"
               if a.join_keys == "random" else "dense keys 3i+1 (round-2 distribution)")
    return {"workload": f"{n:.0e}-row int64 probe x {nb_rows:.0e}-row build inner hash join (probe phase timed), {keydesc}", "rows": n,
            "join_keys": a.join_keys, "partition_mode": {"speculative": a.join_spec, "early_loads": a.join_early_loads, "probe_kernel": a.join_probe_kernel},
            "ms_per_step": ms_per_step, "rows_per_s": n / sec, "dtype": "int64", "build_ms": build_ms, "build_call_ms": build_call_ms,
            "build_plus_probe_ms": build_ms + ms_per_step,  # what the reference's own benchmark times (join_common.hpp:83-122)
            "build_rows_per_s": nb_rows / (build_ms * 1e-3),
            "partition_bits": part_bits, "roofline": roofline, "cpu_baseline": cpu,
            "checked": ("UNCHECKED (--join-unchecked: an ablation measurement, not a result)" if a.join_unchecked else
                        "pairs == closed form; every pair joins equal keys; sum / sum of squares of the matched probe rows")}


# ------------------------------------------------------------------------------------------------
# config 4: groupby(int32 key, 1e6 groups).agg(f64 sum, count)
# ------------------------------------------------------------------------------------------------

def bench_groupby(c):
    a, lib, L, ops, np, torch = c.args, c.lib, c.L, c.ops, c.np, c.torch
    n = c.n
    lib.gx_groupby_set_algorithm(a.gb_algo, a.gb_split)
    lib.gx_groupby_set_partition_mode(a.gb_spec)
    lib.gx_groupby_set_dense(a.gb_dense)
    L.check(lib.gx_groupby_set_partition_bits(a.gb_pbits), "gx_groupby_set_partition_bits")
    gk = ops.random_column(np.int32, n, seed=7 + c.rank, lo=0, hi=1_000_000)
    gv = ops.random_column(np.float64, n, seed=8 + c.rank)
    kdt, ktorch = np.int32, torch.int32
    if a.gb_keys != "dense" and not c.sharded:
        # sparse keys: the dense ids through a mixing BIJECTION (still exactly 1e6 groups, same group sizes), so the LDS tables
        # see keys that hash like random numbers instead of the collision-free dense integers
        ids = c.as_tensor(gk, torch.int32).to(torch.int64)
        if a.gb_keys == "random":
            x = ids & 0xFFFFFFFF
            x = ((x ^ (x >> 16)) * 0x85EBCA6B) & 0xFFFFFFFF
            x = ((x ^ (x >> 13)) * 0xC2B2AE35) & 0xFFFFFFFF
            x = x ^ (x >> 16)
            c.as_tensor(gk, torch.int32).copy_(torch.where(x >= 2**31, x - 2**32, x).to(torch.int32))
        else:
            kdt, ktorch = np.int64, torch.int64
            gk = c.Column.empty(np.int64, n)
            c.as_tensor(gk, torch.int64).copy_(lsr_mix64(ids))
        del ids
    if c.sharded:
        from cudf_amd import distributed as D
        dgk, dgv = c.as_tensor(gk, torch.int32), c.as_tensor(gv, torch.float64)
        step, impl = sharded_step(c, "groupby", lambda: D.distributed_groupby_sum_count(dgk, dgv),   # gxd_groupby_sum_count
                                  lambda: D.distributed_groupby_sum_count(dgk, dgv, local=D.HipLocalOps()))
        sec = c.timed(step)
        k, s, cnt = step()
        tot = cnt.sum().to(torch.int64).reshape(1)
        c.dist.all_reduce(tot)
        assert int(tot.item()) == n * c.world, "distributed groupby: counts do not add up"
        ng = torch.tensor([k.numel()], device="cuda", dtype=torch.int64)
        c.dist.all_reduce(ng)
        assert int(ng.item()) == 1_000_000 or n < 20_000_000, f"distributed groupby: {int(ng.item())} groups over all ranks"
        tv = torch.stack([s.sum(), dgv.sum()])
        c.dist.all_reduce(tv)
        assert abs(float(tv[0].item()) - float(tv[1].item())) <= 1e-9 * abs(float(tv[1].item())), "distributed groupby: sums do not add up"
        return {"workload": f"{n:.0e}-row-per-GPU groupby(int32 key, 1e6 groups).agg(f64 sum,count), partials exchanged [{impl}]",
                "rows": n, "ms_per_step": sec * 1e3, "rows_per_s": n * c.world / sec, "dtype": "f64", "roofline": None,
                "cpu_baseline": None, "checked": "sum of counts == rows, 1e6 groups and the total of the sums over all ranks (every group on one rank)"}
    mg = 1 << 20
    ok, osum = c.Column.empty(kdt, mg), c.Column.empty(np.float64, mg)
    ocv = c.Column.empty(np.int32, mg)
    ng = torch.zeros(1, dtype=torch.int64, device="cuda")
    nb = ctypes.c_size_t(0)
    fn = lambda tmp, nbp: lib.gx_groupby_sum_count(gk.gx, gk.data_ptr, None, gv.gx, gv.data_ptr, None, n, mg,
                                                   ok.data_ptr, osum.data_ptr, ocv.data_ptr, None, c.ptr(ng), tmp, nbp, c.stream)
    L.check(fn(None, ctypes.byref(nb)), "size query")
    tmp = c.device_bytes(nb.value)
    step = lambda: L.check(fn(c.ptr(tmp), ctypes.byref(nb)), "groupby")
    sec = c.timed(step)
    ms_per_step = sec * 1e3
    pinfo = (ctypes.c_int32 * 4)()
    L.check(lib.gx_groupby_plan_info(c.ptr(tmp), mg, pinfo, c.stream), "gx_groupby_plan_info")
    dense_path = bool(pinfo[0]) and not pinfo[1]
    # ---- guard: counts add up to n, keys are distinct and in range, and sampled groups match a direct
    # device-side recomputation (count exact, f64 sum to 1e-11 relative: the kernel's own bar is 1 ulp)
    groups = int(ng.item())
    kt = c.as_tensor(ok, ktorch)[:groups]
    st = c.as_tensor(osum, torch.float64)[:groups]
    ct = c.as_tensor(ocv, torch.int32)[:groups]
    assert int(ct.to(torch.int64).sum().item()) == n, "groupby: counts do not add up to the row count"
    if a.gb_keys == "dense":
        assert int(kt.min().item()) >= 0 and int(kt.max().item()) < 1_000_000, "groupby: key out of range"
    assert int(torch.unique(kt).numel()) == groups, "groupby: duplicate group keys"
    gkt, gvt = c.as_tensor(gk, ktorch), c.as_tensor(gv, torch.float64)
    total_ref = float(gvt.sum().item())
    assert abs(float(st.sum().item()) - total_ref) <= 1e-9 * abs(total_ref), "groupby: sums do not add up"
    for gi in (0, groups // 3, groups - 1):
        key = int(kt[gi].item())
        sel = gkt == key
        assert int(sel.sum().item()) == int(ct[gi].item()), "groupby: sampled group count differs"
        ref = float(gvt[sel].sum().item())
        assert abs(float(st[gi].item()) - ref) <= 1e-11 * max(1.0, abs(ref)), "groupby: sampled group sum differs"
    ach = 12 * n / (ms_per_step * 1e-3) / 1e9
    roofline = {"bound": "hbm",
                "kernel": ("k_slot_sample + k_part_scatter<dense> + k_dense_aggregate (id-range partitions, 10-byte rows, LDS table indexed by the id's remainder)" if dense_path else
                           "k_slot_sample + k_part_scatter + k_part_aggregate (LDS-partitioned groupby, slots sized from a sample)" if a.gb_spec else
                           "k_part_hist + k_part_scatter + k_part_aggregate (LDS-partitioned groupby)"),
                "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS, "traffic": None,
                "traffic_key": "groupby" if a.gb_spec else "groupby (exact two-pass)",
                "algorithmic_bytes_per_launch": 12 * n, "avg_launch_ms": ms_per_step, "groups": groups,
                "path": {"dense_direct_address": int(pinfo[0]), "fell_back_to_exact": int(pinfo[1]), "partition_bits": int(pinfo[2]), "ids_per_partition": int(pinfo[3])},
                "model": "12 B/row (4-B key + 8-B value read once; SURVEY.md 8d)"}
    pmc_traffic(roofline, n)
    cpu = None
    if a.cpu and c.rank == 0:
        cpu = cpu_baseline_groupby(a.cpu_rows or 3e8, a.cpu_rows_pandas or 1e8)
    kdesc = {"dense": "int32 key", "random": "sparse int32 key", "random64": "sparse int64 key"}[a.gb_keys]
    return {"workload": f"{n:.0e}-row groupby({kdesc}, 1e6 groups).agg(float64 sum,count)", "rows": n,
            "ms_per_step": ms_per_step, "rows_per_s": n / sec, "dtype": "f64", "roofline": roofline, "cpu_baseline": cpu,
            "checked": "sum(count) == rows; distinct in-range keys; total and 3 sampled groups recomputed on the device"}


def bench_groupby_minmax(c):
    """groupby(int32 key, 1e6 groups).agg(f64 min, max): the LDS-partitioned MIN / MAX path (gx_groupby_min_max)"""
    a, lib, L, ops, np, torch = c.args, c.lib, c.L, c.ops, c.np, c.torch
    n = c.n
    lib.gx_groupby_set_algorithm(a.gb_algo, a.gb_split)
    lib.gx_groupby_set_partition_mode(a.gb_spec)
    gk = ops.random_column(np.int32, n, seed=7 + c.rank, lo=0, hi=1_000_000)
    gv = ops.random_column(np.float64, n, seed=8 + c.rank)
    mg = 1 << 20
    ok, omin, omax = c.Column.empty(np.int32, mg), c.Column.empty(np.float64, mg), c.Column.empty(np.float64, mg)
    ocv = c.Column.empty(np.int32, mg)
    ng = torch.zeros(1, dtype=torch.int64, device="cuda")
    nb = ctypes.c_size_t(0)
    fn = lambda tmp, nbp: lib.gx_groupby_min_max(gk.gx, gk.data_ptr, None, gv.gx, gv.data_ptr, None, n, mg, ok.data_ptr,
                                                 omin.data_ptr, omax.data_ptr, ocv.data_ptr, c.ptr(ng), tmp, nbp, c.stream)
    L.check(fn(None, ctypes.byref(nb)), "size query")
    tmp = c.device_bytes(nb.value)
    step = lambda: L.check(fn(c.ptr(tmp), ctypes.byref(nb)), "groupby min/max")
    sec = c.timed(step)
    groups = int(ng.item())
    kt = c.as_tensor(ok, torch.int32)[:groups]
    ct = c.as_tensor(ocv, torch.int32)[:groups]
    mnt, mxt = c.as_tensor(omin, torch.float64)[:groups], c.as_tensor(omax, torch.float64)[:groups]
    assert int(ct.to(torch.int64).sum().item()) == n, "groupby min/max: counts do not add up to the row count"
    assert int(torch.unique(kt).numel()) == groups, "groupby min/max: duplicate group keys"
    gkt, gvt = c.as_tensor(gk, torch.int32), c.as_tensor(gv, torch.float64)
    assert float(mnt.min().item()) == float(gvt.min().item()) and float(mxt.max().item()) == float(gvt.max().item())
    for gi in (0, groups // 3, groups - 1):
        sel = gkt == int(kt[gi].item())
        assert float(gvt[sel].min().item()) == float(mnt[gi].item()) and float(gvt[sel].max().item()) == float(mxt[gi].item()), \
            "groupby min/max: sampled group differs"
    ach = 12 * n / sec / 1e9
    roofline = {"bound": "hbm", "traffic_key": "groupby_minmax", "kernel": "k_part_hist + k_part_scatter + k_part_minmax (LDS-partitioned groupby MIN/MAX)",
                "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS, "traffic": None,
                "algorithmic_bytes_per_launch": 12 * n, "avg_launch_ms": sec * 1e3, "groups": groups,
                "model": "12 B/row (4-B key + 8-B value read once; SURVEY.md 8d)"}
    return {"workload": f"{n:.0e}-row groupby(int32 key, 1e6 groups).agg(float64 min,max)", "rows": n, "ms_per_step": sec * 1e3,
            "rows_per_s": n / sec, "dtype": "f64", "roofline": roofline, "cpu_baseline": None,
            "checked": "sum(count) == rows; distinct keys; global min / max and 3 sampled groups recomputed on the device"}


def bench_multikey(c, which):
    """Two int64 key columns (16-byte rows): the hash-and-verify row keys (gx_hash_rows64 + the single-key kernels +
    gx_rows_mismatch_count) against nothing but their own roofline -- the earlier encoding ran one radix sort per key
    column.  join: 1e8-row build side hashed and built once (untimed, like the single-key line), timed = hash the
    probe rows, partitioned probe, certify the pairs.  groupby: timed = ids (hash, distinct keys + first rows, lookup,
    certify) + SUM/COUNT by id + gather of the group keys."""
    a, lib, L, ops, np, torch = c.args, c.lib, c.L, c.ops, c.np, c.torch
    n = c.n
    if which == "join_multikey":
        nb_rows = max(1, n // 10)
        b0 = c.Column.empty(np.int64, nb_rows)
        torch.manual_seed(4242)
        c.as_tensor(b0, torch.int64).copy_(torch.randperm(nb_rows, device="cuda"))          # distinct first column
        b1 = ops.random_column(np.int64, nb_rows, seed=5, lo=0, hi=1 << 40)
        p0 = ops.random_column(np.int64, n, seed=6, lo=0, hi=int(nb_rows / 0.3))          # 30 % of the probe rows hit ...
        p0t, b0t, b1t = c.as_tensor(p0, torch.int64), c.as_tensor(b0, torch.int64), c.as_tensor(b1, torch.int64)
        p1 = c.Column.empty(np.int64, n)
        p1t = c.as_tensor(p1, torch.int64)
        inv = torch.empty(nb_rows, dtype=torch.int64, device="cuda")
        inv[b0t] = torch.arange(nb_rows, device="cuda")
        hit = p0t < nb_rows
        p1t.fill_(-1)
        p1t[hit] = b1t[inv[p0t[hit]]]                                                        # ... with BOTH columns equal
        half = hit & ((p0t & 1) == 1)
        p1t[half] += 1                                                                       # odd keys: second column differs
        expected = int((hit & ~half).sum().item())
        del inv, hit, half
        bk = ops.hash_rows64([b0, b1])
        hj = ops.HashJoin(bk)
        res = {}

        def step():
            pk = ops.hash_rows64([p0, p1])
            l, r = hj.inner_join(pk)
            res["bad"] = ops.rows_mismatch_count([p0, p1], [b0, b1], l, r, l.size)
            res["pairs"] = l.size
        sec = c.timed(step)
        assert res["bad"] == 0 and res["pairs"] == expected, (res, expected)
        bpr = 16 + 8 + 20                      # read 2 keys, write the hash; the single-key join's 20 B/row model
        kname = "gx_hash_rows64 + partitioned probe + gx_rows_mismatch_count (2 x int64 keys)"
        wl = f"{n:.0e}-row probe x {nb_rows:.0e}-row build inner join on 2 int64 key columns"
        checked = "pair count == closed form (rows equal in both columns); every pair certified column by column"
    else:
        k0 = ops.random_column(np.int64, n, seed=21, lo=0, hi=1000)
        k1 = ops.random_column(np.int64, n, seed=22, lo=0, hi=1000)                         # 1e6 (k0, k1) groups
        gv = ops.random_column(np.float64, n, seed=23)
        res = {}

        def step():
            keys, sm, cv, _ = ops.groupby_sum_count_tables([k0, k1], gv)
            res["out"] = (keys, sm, cv)
        sec = c.timed(step)
        keys, sm, cv = res["out"]
        g = sm.size
        assert g == 1_000_000 or n < 20_000_000, g
        assert int(c.as_tensor(cv, torch.int32)[:g].to(torch.int64).sum().item()) == n
        kt0, kt1 = c.as_tensor(keys[0], torch.int64)[:g], c.as_tensor(keys[1], torch.int64)[:g]
        assert int(torch.unique(kt0 * 1000 + kt1).numel()) == g, "duplicate group keys"
        t0, t1, tv = c.as_tensor(k0, torch.int64), c.as_tensor(k1, torch.int64), c.as_tensor(gv, torch.float64)
        for gi in (0, g // 2, g - 1):
            sel = (t0 == int(kt0[gi].item())) & (t1 == int(kt1[gi].item()))
            ref = float(tv[sel].sum().item())
            assert abs(float(c.as_tensor(sm, torch.float64)[gi].item()) - ref) <= 1e-11 * max(1.0, abs(ref))
        bpr = 16 + 8
        kname = "k_wide_scatter + k_wide_aggregate (one partition pass, rows compared in the LDS tables; 2 x int64 keys)"
        wl = f"{n:.0e}-row groupby(2 int64 key columns, 1e6 groups).agg(float64 sum,count)"
        checked = "sum(count) == rows; distinct key pairs; 3 sampled groups recomputed on the device"
    ach = bpr * n / sec / 1e9
    roofline = {"bound": "hbm", "kernel": kname, "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                "traffic": None, "algorithmic_bytes_per_launch": bpr * n, "avg_launch_ms": sec * 1e3,
                "model": f"{bpr} B/row: the key and value columns read once" + (", 8-B hash written, 20 B/row single-key join" if which == "join_multikey" else "")}
    return {"workload": wl, "rows": n, "ms_per_step": sec * 1e3, "rows_per_s": n / sec, "dtype": "int64", "roofline": roofline,
            "cpu_baseline": None, "checked": checked}


def bench_sort_table(c, which):
    """cudf::sorted_order of a 2 x int64 table (one word sort on a nested rank of the tuple, gx_sorted_order_table) and
    cudf::sort_by_key of an 8-byte value column by one int64 key column (sorted_order + gather: src/sort/sort.cu:31-50).  Verified on the
    device every run: the output is a permutation whose (key tuple, row) sequence is strictly increasing -- sortedness AND stability."""
    a, lib, L, ops, np, torch = c.args, c.lib, c.L, c.ops, c.np, c.torch
    n = c.n
    import ctypes
    if which == "sorted_order_table":
        if a.table_keys == "lowcard":
            k0 = ops.random_column(np.int64, n, seed=31, lo=0, hi=1000)
            k1 = ops.random_column(np.int64, n, seed=32)
            kd = "1000 distinct leading values x random 64-bit second column"
        elif a.table_keys == "random":
            k0 = ops.random_column(np.int64, n, seed=31)
            k1 = ops.random_column(np.int64, n, seed=32, lo=0, hi=5)
            kd = "random 64-bit leading column x 5 distinct values"
        else:
            k0 = ops.random_column(np.int64, n, seed=31, lo=0, hi=10)
            k1 = ops.random_column(np.int64, n, seed=32, lo=0, hi=100)
            kd = "10 x 100 distinct values"
        out = c.Column.empty(np.int32, n)
        dt = (ctypes.c_int * 2)(k0.gx, k1.gx)
        dp = (ctypes.c_void_p * 2)(k0.data_ptr, k1.data_ptr)
        de = (ctypes.c_int * 2)(0, 0)
        nb = ctypes.c_size_t(0)
        L.check(lib.gx_sorted_order_table(2, dt, dp, de, n, None, None, ctypes.byref(nb), c.stream), "query")
        tmp = c.device_bytes(nb.value)

        def step():
            L.check(lib.gx_sorted_order_table(2, dt, dp, de, n, out.data_ptr, c.ptr(tmp), ctypes.byref(nb), c.stream), "gx_sorted_order_table")
        sec = c.timed(step)
        st = ctypes.c_int(0)
        L.check(lib.gx_sort_status(c.ptr(tmp), ctypes.byref(st), c.stream), "status")
        assert st.value != 5
        info = (ctypes.c_int32 * 5)()
        L.check(lib.gx_sort_order_map_info(c.ptr(tmp), n, info, c.stream), "info")
        del tmp
        torch.cuda.empty_cache()
        o = c.as_tensor(out, torch.int32)
        assert int(o.to(torch.int64).sum().item()) == n * (n - 1) // 2 and int(o.min().item()) == 0 and int(o.max().item()) == n - 1
        # strictly increasing (k0, k1, row) along the output, checked in slices (the gathers are 8 GB each at 1e9 rows)
        t0, t1 = c.as_tensor(k0, torch.int64), c.as_tensor(k1, torch.int64)
        step_rows = 1 << 27
        for lo in range(0, n, step_rows):
            hi = min(n, lo + step_rows + 1)
            idx = o[lo:hi].to(torch.int64)
            x0, x1 = t0[idx], t1[idx]
            ok = (x0[:-1] < x0[1:]) | ((x0[:-1] == x0[1:]) & ((x1[:-1] < x1[1:]) | ((x1[:-1] == x1[1:]) & (idx[:-1] < idx[1:]))))
            assert bool(ok.all().item()), f"rows {lo}..{hi}: not in (key tuple, row) order"
            del idx, x0, x1, ok
        bpr = 16 + 4
        kname = "gx_sorted_order_table (k_omt_map x 2 + keys-only word sort + k_om_finish_a + k_omt_finish_b)"
        wl = f"{n:.0e}-row sorted_order of a 2 x int64 table, {kd} (one word sort on a nested rank + tuple fix-up of equal-rank runs)"
        checked = "permutation (index sum, min, max); (k0, k1, row) strictly increasing along the whole output"
        extra = {"long_runs": int(info[0]), "row_bits": int(info[2]), "rank_bits": int(info[3])}
    else:
        k = ops.random_column(np.int64, n, seed=41)
        v = ops.random_column(np.int64, n, seed=42)
        res = {}

        def step():
            res["out"] = ops.sort_by_key([v], k)[0]
        sec = c.timed(step)
        o = res["out"]
        # the values arrive in key order: spot slices gathered back through a fresh order
        order = ops.sorted_order(k)
        ot, kt, vt = c.as_tensor(order, torch.int32), c.as_tensor(k, torch.int64), c.as_tensor(v, torch.int64)
        got = c.as_tensor(o, torch.int64)
        for lo in (0, n // 2, max(0, n - (1 << 24))):
            idx = ot[lo:lo + (1 << 24)].to(torch.int64)
            assert bool((got[lo:lo + (1 << 24)] == vt[idx]).all().item())
            ks = kt[idx]
            assert bool((ks[:-1] <= ks[1:]).all().item())
        bpr = 8 + 8 + 8
        kname = "gx_sorted_order (word sort) + gx_gather (8-byte rows through the order)"
        wl = f"{n:.0e}-row sort_by_key (int64 keys, one int64 value column)"
        checked = "3 slices of 2^24 rows: values == values[order], keys[order] non-decreasing"
        extra = {}
    ach = bpr * n / sec / 1e9
    roofline = {"bound": "hbm", "kernel": kname, "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                "traffic": None, "algorithmic_bytes_per_launch": bpr * n, "avg_launch_ms": sec * 1e3,
                "model": f"{bpr} B/row: the key (and value) columns read once, the result written once", **extra}
    return {"workload": wl, "rows": n, "ms_per_step": sec * 1e3, "rows_per_s": n / sec, "dtype": "int64", "roofline": roofline,
            "cpu_baseline": None, "checked": checked}


# ------------------------------------------------------------------------------------------------
# streaming primitives
# ------------------------------------------------------------------------------------------------

def bench_stream(c, which):
    a, lib, L, ops, np, torch = c.args, c.lib, c.L, c.ops, c.np, c.torch
    n = c.n
    src = ops.random_column(np.float64 if which == "reduce" else np.int64, n, seed=11 + c.rank)
    nb = ctypes.c_size_t(0)
    fn = None
    if which == "reduce":
        res = c.Column.empty(np.float64, 1)
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        fn = lambda tmp, nbp: lib.gx_reduce(src.gx, src.data_ptr, None, n, L.OP_SUM, L.FLOAT64, res.data_ptr, c.ptr(cnt), tmp, nbp, c.stream)
        bpr, kname = 8, "gx_reduce f64 SUM"
    elif which == "scan":
        dst = c.Column.empty(np.int64, n)
        fn = lambda tmp, nbp: lib.gx_scan(src.gx, src.data_ptr, None, n, L.OP_SUM, 1, dst.data_ptr, tmp, nbp, c.stream)
        bpr, kname = 16, "gx_scan int64 inclusive SUM"
    else:
        gm = ops.random_column(np.int32, n, seed=13 + c.rank, lo=0, hi=n)
        dst = c.Column.empty(np.int64, n)
        bpr, kname = 20, "gx_gather 8-byte rows through a uniform random int32 map"
    if fn is not None:
        L.check(fn(None, ctypes.byref(nb)), "size query")
        tmp = c.device_bytes(nb.value)
        step = lambda: L.check(fn(c.ptr(tmp), ctypes.byref(nb)), which)
    else:
        step = lambda: L.check(lib.gx_gather(8, src.data_ptr, None, n, gm.data_ptr, n, 0, dst.data_ptr, None, c.stream), "gather")
    sec = c.timed(step)
    checked = None
    if which == "reduce":
        ref = float(c.as_tensor(src, torch.float64).sum().item())
        got = float(res.to_numpy()[0])
        assert abs(got - ref) <= 1e-9 * abs(ref) + 1e-3, "reduce: sum differs from the device recomputation"
        checked = "sum vs torch.sum of the same column"
    elif which == "scan":
        s, d = c.as_tensor(src, torch.int64), c.as_tensor(dst, torch.int64)
        assert int(d[-1].item()) == int(s.sum().item()), "scan: last element is not the wrapped total"
        i = n // 2
        assert int(d[i].item()) - int(d[i - 1].item()) == int(s[i].item()), "scan: adjacent difference differs"
        checked = "last element == wrapped total; adjacent difference at n/2"
    ach = bpr * n / sec / 1e9
    roofline = {"bound": "hbm", "kernel": kname, "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": ach / HBM_PEAK_GBS,
                "traffic": None, "algorithmic_bytes_per_launch": bpr * n, "avg_launch_ms": sec * 1e3}
    return {"workload": f"{n:.0e}-row {kname}", "rows": n, "ms_per_step": sec * 1e3, "rows_per_s": n * c.world / sec,
            "dtype": "f64" if which == "reduce" else "int64", "roofline": roofline, "cpu_baseline": None, "checked": checked}


def through_cpp(args, c, sort_ms, order_ms, join_ms, groupby_ms):
    """What a caller of include/cudf/*.hpp pays (allocation through the pooled mr, result columns, the size read of
    the join) next to the C-ABI numbers of this run: the same workloads through cudf::sort / cudf::sorted_order /
    cudf::hash_join::inner_join / cudf::groupby::aggregate (cpp/include/cudf/sorting.hpp:103-108 and friends), in a
    process of its own (tests/cpp/cudf_api_bench, built by __graft_entry__.build()), wall-clock per call."""
    import subprocess
    exe = os.path.join(ROOT, "tests", "cpp", "cudf_api_bench")
    if not os.path.exists(exe):
        return {"error": "tests/cpp/cudf_api_bench is missing: run `python __graft_entry__.py` (build) first"}
    c.torch.cuda.synchronize()
    c.torch.cuda.empty_cache()
    try:
        out = subprocess.run([exe, str(c.n), str(args.steps), str(args.warmup)], check=True, capture_output=True, text=True,
                             timeout=600).stdout.strip().splitlines()[-1]
        r = json.loads(out)
    except Exception as e:  # noqa: BLE001 -- context, never the headline
        return {"error": repr(e)}
    for k, ref in (("sort", sort_ms), ("sorted_order", order_ms), ("join_probe", join_ms), ("groupby", groupby_ms)):
        if ref and r.get(k + "_ms"):
            r[k + "_vs_c_abi"] = r[k + "_ms"] / ref
    r["note"] = ("wall-clock per call through the C++ API (allocation of outputs and scratch from the pooled mr included); "
                 "the C-ABI numbers beside it use caller-owned buffers")
    return r


def sort_robustness(c, uniform_ms):
    """cudf::sort's cost must not depend on the VALUES (cub::DeviceRadixSort behind cpp/src/sort/sort_radix.cu:52-161 does not care;
    the reference's own benchmark draws keys from [100, 10001): cpp/benchmarks/sort/sort.cpp:24-26).  The same 1e9-row int64 sort on
    distributions the headline is not tuned for, 3 timed steps each, every output checked like the headline's; `ratio` is to the
    uniform line of this run."""
    import copy
    a0 = c.args
    cases = [("normal N(0, 2^40)", {"key_dist": "normal"}), ("lognormal exp(N(25, 3))", {"key_dist": "lognormal"}),
             ("zipf-like floor(u^-5)", {"key_dist": "zipf"}), ("two clusters", {"key_dist": "clusters"}),
             ("uniform in [-1e12, 1e12)", {"key_range": [-10**12, 10**12]}), ("uniform in [100, 10001)", {"key_range": [100, 10001]}),
             ("1e8 copies of one value", {"hot_copies": 1e8}), ("already sorted", {"key_dist": "sorted"}),
             ("float64 N(0, 1)", {"key_type": "float64", "key_dist": "normal"}), ("float64 U[0, 1)", {"key_type": "float64", "key_dist": "uniform"})]
    out, worst = {}, None
    for name, kw in cases:
        a = copy.copy(a0)
        a.steps, a.warmup, a.key_dist, a.key_range, a.hot_copies, a.key_type = 3, 1, "uniform", None, 0, "int64"
        a.full = True   # the guard of every case, and its path from the profiled call
        for k, v in kw.items():
            setattr(a, k, v)
        c.args = a
        try:
            c.torch.cuda.empty_cache()
            b = bench_sort(c, cpu_leg=False)
            si = (b.get("roofline") or {}).get("sort_info") or {}
            out[name] = {"ms_per_step": b["ms_per_step"], "ratio_to_uniform": b["ms_per_step"] / uniform_ms,
                         "path": {"cursor_path_state": si.get("cursor_path_state"), "splitters": (si.get("splitters") or {}).get("on"),
                                  "lsd_passes": si.get("lsd_passes"), "keys_through_big_cells": (si.get("big_cells") or {}).get("keys")}}
            if worst is None or out[name]["ratio_to_uniform"] > worst[1]:
                worst = (name, out[name]["ratio_to_uniform"])
        except Exception as e:  # noqa: BLE001 -- a robustness line must not take the headline down; it says what happened
            out[name] = {"error": repr(e)}
        finally:
            c.args = a0
    return {"rows": c.n, "steps": 3, "warmup": 1, "uniform_ms": uniform_ms, "cases": out,
            "worst": {"case": worst[0], "ratio_to_uniform": worst[1]} if worst else None,
            "checked": "every case: order + multiset checksum of the timed output (gx_checksum), as the headline",
            "state_legend": "cursor_path_state 3 = two partition levels + cell sort (splitters: level 0 cut on sample-chosen splitters), "
                            "5 = counting sort of a narrow range, 4 / 2 = declined to the LSD passes / look-back path"}


def sorted_order_robustness(c, uniform_ms):
    """The same for cudf::sorted_order -- what sort_by_key, the sort-path groupby, multi-column sorts and DataFrame.sort_values sit on
    (cub's SortPairs behind cpp/src/sort/sorted_order_radix.cu:56-179 costs the same on any distribution).  Every
    output verified like the headline sorted_order run: a permutation, keys gathered through it sorted + multiset, ties in row order."""
    import copy
    a0 = c.args
    cases = [("normal N(0, 2^40)", {"key_dist": "normal"}), ("lognormal exp(N(25, 3))", {"key_dist": "lognormal"}),
             ("zipf-like floor(u^-5)", {"key_dist": "zipf"}), ("two clusters", {"key_dist": "clusters"}),
             ("uniform in [-1e12, 1e12)", {"key_range": [-10**12, 10**12]}), ("uniform in [100, 10001)", {"key_range": [100, 10001]}),
             ("1e8 copies of one value", {"hot_copies": 1e8}), ("already sorted", {"key_dist": "sorted"}),
             ("float64 N(0, 1)", {"key_type": "float64", "key_dist": "normal"}), ("float64 U[0, 1)", {"key_type": "float64", "key_dist": "uniform"})]
    out, worst = {}, None
    for name, kw in cases:
        a = copy.copy(a0)
        a.steps, a.warmup, a.key_dist, a.key_range, a.hot_copies, a.key_type = 3, 1, "uniform", None, 0, "int64"
        a.full = True   # the guard of every case, and its path from the profiled call
        for k, v in kw.items():
            setattr(a, k, v)
        c.args = a
        try:
            c.torch.cuda.empty_cache()
            b = bench_sort(c, pairs=True, cpu_leg=False)
            r = b.get("roofline") or {}
            si = r.get("sort_info") or {}
            out[name] = {"ms_per_step": b["ms_per_step"], "ratio_to_uniform": b["ms_per_step"] / uniform_ms,
                         "path": {"word_sort_cursor_path_state": si.get("cursor_path_state"), "splitters": (si.get("splitters") or {}).get("on"),
                                  "lsd_passes": si.get("lsd_passes"), "order_map": r.get("order_map")}}
            if worst is None or out[name]["ratio_to_uniform"] > worst[1]:
                worst = (name, out[name]["ratio_to_uniform"])
        except Exception as e:  # noqa: BLE001 -- a robustness line must not take the headline down; it says what happened
            out[name] = {"error": repr(e)}
        finally:
            c.args = a0
    return {"rows": c.n, "steps": 3, "warmup": 1, "uniform_ms": uniform_ms, "cases": out,
            "worst": {"case": worst[0], "ratio_to_uniform": worst[1]} if worst else None,
            "checked": "every case: the timed int32 order is a permutation of [0, n); keys gathered through it: order + multiset checksum; equal keys in row order"}


def main():
    args = parse()
    if args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(spawn_ranks(args))
    c = Ctx(args)
    if c.world != max(1, args.gpus) and c.rank == 0:
        print(f"bench.py: note: --gpus {args.gpus} but the process group has {c.world} rank(s); n_gpus reports the group", file=sys.stderr)
    wl = args.workload
    blocks = {}
    if c.sharded:
        if c.world > 1:
            start_heartbeat_monitor(c)
        if wl in ("all", "sort", "join", "groupby") or args.preflight_only:
            c.preflight = preflight(c)
            if c.rank == 0:
                print("bench.py: pre-flight of the sharded operators: " + json.dumps(c.preflight), file=sys.stderr, flush=True)
        if args.preflight_only:
            if c.rank == 0:
                print(json.dumps({"preflight": c.preflight, "n_gpus": c.world}), flush=True)
            from cudf_amd import distributed as D
            D.close_communicators()
            c.dist.destroy_process_group()
            bad = [k for k in ("sort_fused", "sort_sample", "join", "groupby") if not str(c.preflight.get(k, "")).startswith("ok")]
            sys.exit(1 if bad else 0)
    if wl in ("all", "sort", "sorted_order"):
        head = bench_sort(c, pairs=(wl == "sorted_order"), dump=bool(args.dump_outputs))
        if wl == "all" and args.full:
            if not c.sharded:  # cudf::sorted_order, what the reference's sort benchmark times (cpp/benchmarks/sort/sort.cpp:16-58): its own block
                c.torch.cuda.empty_cache()
                blocks["sorted_order"] = bench_sort(c, pairs=True, cpu_leg=False)
            c.torch.cuda.empty_cache()
            blocks["join"] = bench_join(c)
            c.torch.cuda.empty_cache()
            blocks["groupby"] = bench_groupby(c)
    elif wl == "join":
        head = bench_join(c)
    elif wl == "groupby":
        head = bench_groupby(c)
    elif wl == "groupby_minmax":
        head = bench_groupby_minmax(c)
    elif wl in ("join_multikey", "groupby_multikey"):
        head = bench_multikey(c, wl)
    elif wl in ("sorted_order_table", "sort_by_key"):
        head = bench_sort_table(c, wl)
    else:
        head = bench_stream(c, wl)
    if c.rank == 0:
        line = {
            "metric": METRIC, "value": head["rows_per_s"], "unit": "rows/s", "n_gpus": c.world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": head["ms_per_step"], "higher_is_better": True, "scaling": "weak", "full": args.full,
            "vs_baseline": None, "dtype": head["dtype"], "data": "synthetic",
            "config": {"workload": head["workload"], "rows_per_gpu": c.n, "algo": args.algo, "gb_algo": args.gb_algo, "gb_spec": args.gb_spec, "gb_pbits": args.gb_pbits, "gb_keys": args.gb_keys,
                       "parallelism": (f"{c.world} ranks, row shards, one all-to-all exchange per step (RCCL over xGMI)"
                                       if c.world > 1 else ("1 GPU, the sharded operators with the exchange forced (--force-sharded)" if c.sharded else "1 GPU"))},
            "roofline": head["roofline"], "cpu_baseline": head["cpu_baseline"], "checked": head.get("checked"),
        }
        if c.preflight is not None:
            line["preflight"] = c.preflight   # the sharded operators against the oracle on this run's transport, before anything was timed
        for k in ("build_ms", "build_call_ms", "build_plus_probe_ms", "build_rows_per_s", "partition_bits", "matches", "join_keys", "partition_mode"):
            if k in head:
                line["join_" + k if not k.startswith("join") else k] = head[k]
        for name, b in blocks.items():
            line[name] = {"config": {"workload": b["workload"]}, "value": b["rows_per_s"], "unit": "rows/s",
                          "ms_per_step": b["ms_per_step"], "steps": args.steps, "warmup": args.warmup, "dtype": b["dtype"],
                          "roofline": b["roofline"], "cpu_baseline": b["cpu_baseline"], "checked": b.get("checked"),
                          **({"build_ms": b["build_ms"], "build_call_ms": b.get("build_call_ms"), "build_plus_probe_ms": b.get("build_plus_probe_ms"),
                              "build_rows_per_s": b.get("build_rows_per_s"), "partition_bits": b["partition_bits"], "join_keys": b.get("join_keys"),
                              "partition_mode": b.get("partition_mode")} if "build_ms" in b else {})}
        want_rb = args.robustness if args.robustness is not None else (args.full and wl == "all" and c.n >= 100_000_000)
        if want_rb and not c.sharded and wl in ("all", "sort"):
            line["sort_robustness"] = sort_robustness(c, head["ms_per_step"])
            if "sorted_order" in line:
                line["sorted_order_robustness"] = sorted_order_robustness(c, line["sorted_order"]["ms_per_step"])
        if args.robustness and not c.sharded and wl == "sorted_order":
            line["sorted_order_robustness"] = sorted_order_robustness(c, head["ms_per_step"])
        want_cpp = args.through_cpp if args.through_cpp is not None else (args.full and wl == "all" and c.n >= 100_000_000)
        if want_cpp and not c.sharded:
            blk = lambda name: (blocks.get(name) or (head if wl == name else {})).get("ms_per_step")
            line["through_cpp"] = through_cpp(args, c, head["ms_per_step"] if wl in ("all", "sort") else None, blk("sorted_order"),
                                              blk("join"), blk("groupby"))
        for r in [line.get("roofline")] + [line[k].get("roofline") for k in ("sorted_order", "join", "groupby") if k in line]:
            if not r:
                continue
            # achieved GB/s two ways (model bytes / time, PMC bytes / time), against the 8.0 TB/s spec and
            # against the 6.29 TB/s copy ceiling measured on this part (MI355X_MICROARCH.md)
            r["peak_measured_copy"] = HBM_COPY_GBS
            r["frac_of_measured_copy"] = r["achieved"] / HBM_COPY_GBS
            if r.get("traffic") and r.get("avg_launch_ms"):
                r["traffic_GBps"] = r["traffic"] / (r["avg_launch_ms"] * 1e-3) / 1e9
        print(json.dumps(line), flush=True)
    if c.sharded:
        from cudf_amd import distributed as D
        D.close_communicators()  # the RCCL communicators of the C++ operators, before the process group they were made with
        c.dist.destroy_process_group()


if __name__ == "__main__":
    main()
