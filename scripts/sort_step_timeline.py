"""From a rocprofv3 --kernel-trace results.db of `bench.py --workload sort`: ONE cudf::sort call as a table, one row per kernel
launch in stream order -- kernel | workgroups | duration | gap since the previous launch ended -- and the sums "three streaming
kernels" (level 0, level 1, cell sort) against "everything else" (other kernels + gaps; see the note the table prints about the gap column).
usage: sort_step_timeline.py <db> [step index from the end, default 1 = the last whole step] [title]"""
import re
import sqlite3
import sys


def short(name):
    name = re.sub(r"^void ", "", name)
    name = name.replace("gx::sort::", "").replace("(anonymous namespace)::", "")
    return re.sub(r"\(.*$", "", name)


def main(db, back=1, title=""):
    cur = sqlite3.connect(db).cursor()
    cols = [r[1] for r in cur.execute("pragma table_info(kernels)").fetchall()]
    gx = next((c for c in ("grid_x", "grid_size_x", "grid_size") if c in cols), None)
    wx = next((c for c in ("workgroup_x", "workgroup_size_x", "workgroup_size") if c in cols), None)
    sel = "name, start, end" + (f", {gx}" if gx else ", 0") + (f", {wx}" if wx else ", 1")
    rows = cur.execute(f"select {sel} from kernels order by start").fetchall()
    # a sort call starts with k_hf_sample<.., false> (the cursor path) and its second k_hf_sample is the <.., true> form
    samp = [i for i, r in enumerate(rows) if "k_hf_sample" in r[0]]
    starts = samp[0::2]
    if len(starts) < back + 1:
        print("# not enough sort calls in the trace")
        return
    lo = starts[-back - 1]
    hi = starts[-back]
    step = [r for r in rows[lo:hi] if "gx::sort" in r[0]]
    print(f"# {title}")
    print(f"# one sort call ({len(step)} kernel launches; memsets are not kernels and have no row), stream order; microseconds")
    print("# dur_us = end - start of the dispatch, gap_us = start - end of the previous dispatch.  On an in-order queue the trace's stamps are")
    print("# contiguous (every start is its predecessor's end to within 0.1 us), so gap_us is zero by construction, NOT a measured absence of")
    print("# gaps: the idle time before a kernel is inside ITS dur_us (a launch that returns at once shows as 4.5 - 5 us), and 'everything else'")
    print("# below is kernels and launch gaps together.  The window opens at the first kernel: the memsets enqueued before it (the plan; in")
    print("# builds that clear the cell tables with a memset, those 4 MB too) are outside it.")
    print("%-4s %-92s %9s %10s %9s" % ("#", "kernel", "workgroups", "dur_us", "gap_us"))
    big_total = other = gaps = 0.0
    prev_end = None
    for i, (name, s, e, g, w) in enumerate(step):
        dur = (e - s) / 1e3
        gap = 0.0 if prev_end is None else (s - prev_end) / 1e3
        prev_end = e
        gaps += gap
        if dur > 1000.0:
            big_total += dur
        else:
            other += dur
        wg = (g // w) if (g and w) else 0
        print("%-4d %-92s %9d %10.1f %9.1f" % (i, short(name)[:92], wg, dur, gap))
    wall = (step[-1][2] - step[0][1]) / 1e3
    print(f"# first start to last end: {wall / 1e3:.3f} ms")
    print(f"# three streaming kernels (every launch longer than 1 ms): {big_total / 1e3:.3f} ms")
    print(f"# everything else: {(wall - big_total) / 1e3:.3f} ms = other kernels {other / 1e3:.3f} ms + gaps {gaps / 1e3:.3f} ms")


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 1, " ".join(sys.argv[3:]))
