"""gx_sort_keys of 1e9 uniform int64 keys with the cursor path's FALLBACK forced (gx_sort_set_cursor_path(1, -8.0): every level-0
slot is smaller than its estimate, level 0 overflows, state 2): the one configuration in which the look-back chain runs in the
fallback role, on the bounded grids of role_grid (gx_sort.hip) -- k_msd_pass in its MULTI form, k_local_place / k_local_sort walking
the cells.  Next to it the same chain as the PRIMARY path (cursor path off: one workgroup per ticket / cell) and the cursor path
itself.  Then float64 keys (uniform doubles): a clean column (cursor path) and the same column with ONE NaN in a row the sample does
not read -- level 0 finds it, the cursor path declines (state 2) and the look-back chain, for float keys always in the primary role,
sorts the column.  HIP events around the calls; a checksum / an order check guards every result.
usage: python scripts/xp/xp_sort_forced_fallback.py [rows] [repetitions]"""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np
import torch
import cudf_amd
from cudf_amd import Column, ops, _lib as L

n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1_000_000_000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
sp = ops.stream_ptr()
keys = ops.random_column(np.int64, n, seed=11)
out = Column.empty(np.int64, n)
ref = ops.checksum(keys)
try:
    for name, enable, margin in (("cursor path", 1, 0.0), ("forced fallback", 1, -8.0), ("cursor path off", 0, 0.0)):
        L.lib.gx_sort_set_cursor_path(enable, margin)
        nb = ctypes.c_size_t(0)
        L.check(L.lib.gx_sort_keys(keys.gx, keys.data_ptr, out.data_ptr, n, 0, None, ctypes.byref(nb), sp), "query")
        tmp = ops.device_bytes(nb.value)
        call = lambda: L.check(L.lib.gx_sort_keys(keys.gx, keys.data_ptr, out.data_ptr, n, 0, ops.ptr(tmp), ctypes.byref(nb), sp), "sort")
        call(); call()
        times = []
        for _ in range(reps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize(); s.record()
            call()
            e.record(); torch.cuda.synchronize()
            times.append(s.elapsed_time(e))
        st = ctypes.c_int32(-1)
        L.lib.gx_sort_cursor_state(ops.ptr(tmp), ctypes.byref(st), sp)
        info = (ctypes.c_int32 * 8)()
        L.lib.gx_sort_info(ops.ptr(tmp), info, sp)
        cs = ops.checksum(out)
        assert cs[2] == 0 and cs[:2] == ref[:2], (cs, ref)
        times.sort()
        print(f"sort_keys int64 n={n:.1e} {name:16s} state {st.value} hybrid_used {info[1]} lsd_passes {info[7]} | ms per call: median {times[len(times) // 2]:7.3f} "
              f"min {times[0]:7.3f} max {times[-1]:7.3f} ({reps} calls)", flush=True)
        del tmp
finally:
    L.lib.gx_sort_set_cursor_path(1, 0.0)
del keys, out

fkeys = Column.empty(np.float64, n)
ft = fkeys.data[: n * 8].view(torch.float64)
g = torch.Generator(device="cuda").manual_seed(7)
for i in range(0, n, 1 << 27):
    m = min(1 << 27, n - i)
    ft[i:i + m] = torch.rand(m, generator=g, device="cuda", dtype=torch.float64)
ft[ft == 0] = 1.0
fout = Column.empty(np.float64, n)
ot = fout.data[: n * 8].view(torch.float64)
for name, nan_row in (("float64 clean", -1), ("float64 one NaN", 64 + 5)):  # row 69 is in no sampled chunk (chunks start at multiples of stride * 64)
    if nan_row >= 0:
        ft[nan_row] = float("nan")
    torch.cuda.synchronize()
    nb = ctypes.c_size_t(0)
    L.check(L.lib.gx_sort_keys(fkeys.gx, fkeys.data_ptr, fout.data_ptr, n, 0, None, ctypes.byref(nb), sp), "query")
    tmp = ops.device_bytes(nb.value)
    call = lambda: L.check(L.lib.gx_sort_keys(fkeys.gx, fkeys.data_ptr, fout.data_ptr, n, 0, ops.ptr(tmp), ctypes.byref(nb), sp), "sort")
    call(); call()
    times = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); s.record()
        call()
        e.record(); torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    st = ctypes.c_int32(-1)
    L.lib.gx_sort_cursor_state(ops.ptr(tmp), ctypes.byref(st), sp)
    m = n - 1 if nan_row >= 0 else n   # NaN sorts last
    bad = 0
    for i in range(0, m - 1, 1 << 27):
        j = min(i + (1 << 27), m - 1)
        bad += int((ot[i + 1:j + 1] < ot[i:j]).sum())
    assert bad == 0 and (nan_row < 0 or bool(torch.isnan(ot[n - 1]))), (bad, name)
    times.sort()
    print(f"sort_keys {name:16s} n={n:.1e} state {st.value} | ms per call: median {times[len(times) // 2]:7.3f} min {times[0]:7.3f} max {times[-1]:7.3f} ({reps} calls)", flush=True)
    del tmp
print("ok")
