"""NumPy models of the conditional joins (cudf_amd/csrc/gx_conditional_join.hip).

grid_matches: the predicate on the broadcast n_left x n_right grid with the per-value rules of tests/expression_model.py; a pair
matches when the result is valid and true.  join_of: the one-line model of the five kinds in the order gx.h fixes, from that
matrix.  walk_join: the kernel's walk -- tiles of TL left rows under a capped grid, the right table in segments of whole chunks of TR rows
(one workgroup per tile and segment), R pairs per run of the program, a count pass per (row, segment), the place of an unmatched
row, an exclusive scan, a write pass that evaluates again, the early exits of the mark pass -- on the same matrix; tests/test_conditional_join_host.py holds it to join_of exhaustively on a scaled-down shape."""
import numpy as np

from tests import expression_model as M

NO_MATCH = -2**31
KINDS = ("inner", "left", "full", "leftsemi", "leftanti")


def grid_matches(nodes, columns, left, right, lits):
    """bool [n_left, n_right].  nodes / columns: ast.flatten_pair's; left / right: lists of (values, validity) by table index;
    lits: list of (one-element values, one-element validity)"""
    sides = {"left": left, "right": right}
    cols = []
    for table, index in columns:
        v, ok = sides[table][index]
        shape = (-1, 1) if table == "left" else (1, -1)
        cols.append((np.asarray(v).reshape(shape), np.asarray(ok, dtype=bool).reshape(shape)))
    n_left = len(left[0][0]) if left else 0
    n_right = len(right[0][0]) if right else 0
    ty = M.node_types(nodes, [M.GX[c[0].dtype] for c in cols], [M.GX[l[0].dtype] for l in lits])
    assert ty[-1] == M.GX[np.dtype(np.bool_)], "the predicate must be BOOL8"

    def ev(i):
        kind, op, lhs, rhs = nodes[i]
        if kind == M.COLUMN:
            return cols[lhs]
        if kind == M.LITERAL:
            v, ok = lits[lhs]
            return np.asarray(v).reshape(1, 1), np.asarray(ok, dtype=bool).reshape(1, 1)
        a, av = ev(lhs)
        if kind == M.UNARY:
            v, ok = M.unary_value(M.AST_OPS[op], ty[lhs], a, av)
        else:
            b, bv = ev(rhs)
            v, ok = M.binary_value(M.AST_OPS[op], ty[lhs], a, av, b, bv)
        return v.astype(M.NP[ty[i]]), ok

    v, ok = ev(len(nodes) - 1)
    return np.broadcast_to((v != 0) & ok, (n_left, n_right)).copy()


def join_of(m, kind):
    """the join of `kind` from the match matrix: (left, right) int32 arrays, or one array for leftsemi / leftanti"""
    n_left, n_right = m.shape
    any_l = m.any(axis=1) if n_right else np.zeros(n_left, dtype=bool)
    if kind == "leftsemi":
        return np.flatnonzero(any_l).astype(np.int32)
    if kind == "leftanti":
        return np.flatnonzero(~any_l).astype(np.int32)
    l, r = np.nonzero(m)                                         # row-major: ascending (left, right)
    if kind == "inner":
        return l.astype(np.int32), r.astype(np.int32)
    lone = np.flatnonzero(~any_l)
    l2 = np.concatenate([l, lone])
    r2 = np.concatenate([r, np.full(len(lone), NO_MATCH)])
    order = np.lexsort((r2, l2))                                 # an unmatched row has one entry: it lands in its place
    l2, r2 = l2[order], r2[order]
    if kind == "full":
        any_r = m.any(axis=0) if n_left else np.zeros(n_right, dtype=bool)
        tail = np.flatnonzero(~any_r)
        l2 = np.concatenate([l2, np.full(len(tail), NO_MATCH)])
        r2 = np.concatenate([r2, tail])
    return l2.astype(np.int32), r2.astype(np.int32)


def walk_join(m, kind, TL, TR, R, grid_cap, chunks_per_segment=1):
    """the kernel's walk over the match matrix; returns what join_of returns plus the count pass's total as a Python int"""
    n_left, n_right = m.shape
    assert TR % R == 0
    tiles = -(-n_left // TL)
    grid = max(1, min(tiles, grid_cap))
    outer = kind in ("left", "full")
    seg_rows = chunks_per_segment * TR
    n_seg = max(1, -(-n_right // seg_rows))

    def runs(i, seg, on_run, stop=None):
        """the runs of the program of left row i in segment seg: on_run(first right row, match bits of the R pairs)"""
        hi = min(n_right, (seg + 1) * seg_rows)
        for c0 in range(seg * seg_rows, hi, TR):
            rc = min(TR, hi - c0)
            for r0 in range(0, rc, R):
                if stop is not None and stop():
                    return
                ex = min(R, rc - r0)
                on_run(c0 + r0, m[i, c0 + r0:c0 + r0 + ex])

    def rows():
        """(left row, segment) in the order of the workgroups: segments outermost, as blockIdx.y is"""
        for seg in range(n_seg):
            for block in range(grid):
                for tile in range(block, tiles, grid):
                    for t in range(TL):
                        if tile * TL + t < n_left:
                            yield tile * TL + t, seg

    if kind in ("leftsemi", "leftanti"):
        bits = np.full(n_left, kind == "leftanti")              # ANTI starts from ones and clears, SEMI from zeroes and sets
        for i, seg in rows():
            hit = [False]

            def mark(first, mm, hit=hit):
                hit[0] = hit[0] or bool(mm.any())
            runs(i, seg, mark, stop=lambda hit=hit: hit[0])    # the early exit, at its finest: one row of one segment
            if hit[0]:
                bits[i] = kind == "leftsemi"
        out = np.flatnonzero(bits).astype(np.int32)
        return out, len(out)

    counts = np.zeros((n_left, n_seg), dtype=np.int64)
    unmatched = np.ones(n_right, dtype=bool)
    for i, seg in rows():
        c = [0]

        def count(first, mm, c=c):
            c[0] += int(mm.sum())
            if kind == "full":
                unmatched[first:first + len(mm)] &= ~mm
        runs(i, seg, count)
        counts[i, seg] = c[0]
    lone = ~counts.any(axis=1) if outer else np.zeros(n_left, dtype=bool)
    counts[lone, 0] = 1                                          # the one place of a row without a match
    left_total = int(counts.sum())
    flat = counts.reshape(-1)
    offsets = (np.cumsum(flat) - flat).reshape(n_left, n_seg)
    out_l = np.full(left_total, -7, dtype=np.int64)
    out_r = np.full(left_total, -7, dtype=np.int64)
    for i, seg in rows():
        pos = [int(offsets[i, seg])]

        def write(first, mm, pos=pos, i=i):
            for k in np.flatnonzero(mm):
                out_l[pos[0]], out_r[pos[0]] = i, first + k
                pos[0] += 1
        runs(i, seg, write)
        if seg == 0 and lone[i]:
            out_l[offsets[i, 0]], out_r[offsets[i, 0]] = i, NO_MATCH
    total = left_total
    if kind == "full":
        tail = np.flatnonzero(unmatched)
        out_l = np.concatenate([out_l, np.full(len(tail), NO_MATCH)])
        out_r = np.concatenate([out_r, tail])
        total += len(tail)
    return (out_l.astype(np.int32), out_r.astype(np.int32)), total
