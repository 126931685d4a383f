"""GPU: the plain `bench.py` line (set-up, warm-up, timed steps, result line: nothing else), the outputs it writes under
--dump-outputs against a sort of the same seeded input, and the blocks, guards and rooflines that --full adds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_plain_line_and_dumped_outputs(tmp_path):
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from cudf_amd import ops
    n = 5_000_000
    line = _run(["--gpus", "1", "--rows", str(n), "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)], 600)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False and line["unit"] == "rows/s" and line["dtype"] == "int64"
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(n / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert not {"sorted_order", "join", "groupby", "sort_robustness", "through_cpp"} & set(line)
    assert line["cpu_baseline"] is None and line["roofline"] is None
    keys = ops.random_column(np.int64, n, seed=42)                # bench_sort's input: the same seed, the same device RNG
    want = torch.sort(keys.data[: n * 8].view(torch.int64)).values.cpu().numpy()[bench.dump_rows(n)]
    hi = np.load(tmp_path / "sorted_keys_hi32.npy")
    lo = np.load(tmp_path / "sorted_keys_lo32.npy")
    assert hi.dtype == np.float64 and len(hi) == bench.DUMP_ROWS
    np.testing.assert_array_equal((hi.astype(np.int64) << 32) | lo.astype(np.int64), want)


def test_full_line_carries_the_blocks_and_the_guards():
    line = _run(["--gpus", "1", "--rows", "20000000", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline"], 900)
    assert line["full"] is True and line["checked"] and line["roofline"]
    for k in ("sorted_order", "join", "groupby"):
        assert line[k]["checked"] and line[k]["value"] > 0 and line[k]["steps"] == 2, k
