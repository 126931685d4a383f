"""CPU: host logic of bench.py that needs no device -- the order in which Ctx.timed drives the event slots of the kernels' HIP events
(step k records into slot k % 64; every slot is read AFTER the closing barrier: no read-back between two timed steps)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ctx(steps, warmup):
    sys.path.insert(0, ROOT)
    import bench

    class A:
        pass
    a = A()
    a.steps, a.warmup = steps, warmup
    c = bench.Ctx.__new__(bench.Ctx)
    c.args, c.world, c.beat = a, 1, 0.0
    return bench, c


def test_timed_records_into_slots_and_reads_after_the_barrier():
    bench, c = _ctx(5, 2)
    log = []
    c.barrier = lambda: log.append("barrier")
    sec = bench.Ctx.timed(c, lambda: log.append("step"), after_warmup=lambda: log.append("aw"),
                          slot=lambda k: log.append(f"s{k}"), read_slot=lambda: log.append("read"))
    assert sec >= 0.0
    assert log == (["step", "step", "aw", "barrier"] + [x for k in range(5) for x in (f"s{k}", "step")] + ["barrier"] +
                   [x for k in range(5) for x in (f"s{k}", "read")] + ["s0"])


def test_timed_more_steps_than_slots_reads_the_last_launches():
    bench, c = _ctx(bench_steps := 70, 0)
    log = []
    c.barrier = lambda: None
    bench.Ctx.timed(c, lambda: None, slot=lambda k: log.append(k), read_slot=lambda: log.append("r"))
    rec, rd = log[:bench_steps], log[bench_steps:]
    assert rec == [k % bench.PROFILE_SLOTS for k in range(bench_steps)]
    assert rd.count("r") == bench.PROFILE_SLOTS and rd[-1] == 0


def test_timed_without_slots_is_the_plain_contract():
    bench, c = _ctx(3, 1)
    log = []
    c.barrier = lambda: log.append("barrier")
    bench.Ctx.timed(c, lambda: log.append("step"), per_step=lambda: log.append("ps"))
    assert log == ["step", "barrier", "step", "ps", "step", "ps", "step", "ps", "barrier"]


def _parse(monkeypatch, *argv):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_leaves_the_extras_to_full(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.full, a.cpu, a.robustness, a.through_cpp, a.dump_outputs, a.steps, a.warmup) == (False, False, None, None, None, 7, 2)
    a = _parse(monkeypatch, "--full")
    assert a.full and a.cpu
    assert not _parse(monkeypatch, "--full", "--no-cpu-baseline").cpu


def test_parse_rejects_what_it_cannot_do(monkeypatch):
    import pytest
    for argv in (["--steps", "0"], ["--warmup", "-1"], ["--dump-outputs", "d", "--workload", "join"], ["--dump-outputs", "d", "--gpus", "2"]):
        with pytest.raises(SystemExit):
            _parse(monkeypatch, *argv)


def test_dump_rows_is_a_fixed_sample_of_the_whole_output():
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    np.testing.assert_array_equal(bench.dump_rows(1000), np.arange(1000))
    n, m = 10**9, bench.DUMP_ROWS
    r = bench.dump_rows(n)
    np.testing.assert_array_equal(r, bench.dump_rows(n))
    assert len(r) == m and r[0] >= 0 and r[-1] < n and bool((np.diff(r) > 0).all())
    edges = np.arange(m + 1) * n // m
    assert bool((r >= edges[:-1]).all() and (r < edges[1:]).all())   # one row in each of m equal ranges


def test_dump_outputs_are_float64_and_exact(tmp_path):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import bench

    class Col:
        def __init__(self, a):
            self.data, self.size, self.dtype = torch.from_numpy(a.view(np.uint8).copy()), len(a), a.dtype
    c = bench.Ctx.__new__(bench.Ctx)
    c.np, c.torch = np, torch

    class A:
        dump_outputs = str(tmp_path / "out")
    c.args = A()
    keys = np.sort(np.random.default_rng(1).integers(-2**63, 2**63 - 1, 3 * bench.DUMP_ROWS, dtype=np.int64))
    keys[0], keys[-1] = -2**63, 2**63 - 1
    bench.dump_outputs(c, Col(keys), torch.int64)
    hi = np.load(tmp_path / "out" / "sorted_keys_hi32.npy")
    lo = np.load(tmp_path / "out" / "sorted_keys_lo32.npy")
    assert hi.dtype == lo.dtype == np.float64 and len(hi) == bench.DUMP_ROWS
    rows = bench.dump_rows(len(keys))
    np.testing.assert_array_equal((hi.astype(np.int64) << 32) | lo.astype(np.int64), keys[rows])
    order = np.random.default_rng(2).permutation(5000).astype(np.int32)
    bench.dump_outputs(c, Col(order), torch.int32)
    np.testing.assert_array_equal(np.load(tmp_path / "out" / "sorted_order.npy"), order.astype(np.float64))
    f = np.random.default_rng(3).standard_normal(777)
    bench.dump_outputs(c, Col(f), torch.float64)
    assert np.load(tmp_path / "out" / "sorted_keys.npy").tobytes() == f.tobytes()
    total = sum(os.path.getsize(tmp_path / "out" / x) for x in ("sorted_keys_hi32.npy", "sorted_keys_lo32.npy"))
    assert total <= 64 << 20
