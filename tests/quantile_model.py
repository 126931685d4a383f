"""Plain NumPy models of the quantile kernels (cudf_amd/csrc/gx_quantile.hip), shared by test_quantile_host.py and
test_gpu_quantile.py: the sortable words, the index rule, the interpolation in float64, and the select protocol (range, digit,
histogram, plan, candidate positions)."""
import numpy as np

NBINS = 2048
INTERPS = ("linear", "lower", "higher", "midpoint", "nearest")


def sortable_words(a: np.ndarray) -> np.ndarray:
    """unsigned words whose order is the order of the sorts: signed -> sign flip; float -> -0.0 as +0.0, every NaN the greatest
    word, then the total-order flip.  Returned as uint64 (zero-extended)."""
    a = np.ascontiguousarray(a)
    w = a.dtype.itemsize
    u = a.view(np.dtype(f"u{w}")).astype(np.uint64)
    sign = np.uint64(1) << np.uint64(8 * w - 1)
    ones = np.uint64((1 << (8 * w)) - 1)
    if a.dtype.kind == "i":
        return u ^ sign
    if a.dtype.kind == "u":
        return u
    nan = np.isnan(a)
    u = np.where(a == 0, np.uint64(0), u)
    neg = (u & sign) != 0
    out = np.where(neg, ~u & ones, u ^ sign)
    return np.where(nan, ones, out).astype(np.uint64)


def index(count: int, q: float):
    """(lower, higher, nearest, frac) in float64, as the kernels' quantile_index"""
    q = np.float64(min(max(q, 0.0), 1.0))
    pos = q * np.float64(count - 1)
    lower, higher, nearest = int(np.floor(pos)), int(np.ceil(pos)), int(np.rint(pos))
    return lower, higher, nearest, np.float64(pos - np.float64(lower))


def as_double(x) -> np.float64:
    return np.float64(x)


def interpolate(interp: str, a, b, ix) -> np.float64:
    """one rounding per product and per sum: what float64 NumPy scalars do"""
    lower, _, nearest, frac = ix
    da, db = as_double(a), as_double(b)
    with np.errstate(all="ignore"):
        if interp == "linear":
            return np.float64((np.float64(1.0) - frac) * da) + np.float64(frac * db)
        if interp == "midpoint":
            return np.float64(da / np.float64(2.0)) + np.float64(db / np.float64(2.0))
    if interp == "lower":
        return da
    if interp == "higher":
        return db
    return da if nearest == lower else db


def digit_shift(span: int) -> int:
    return 0 if span < NBINS else span.bit_length() - 11


def select_plan(words: np.ndarray, ranks):
    """The select protocol on the sortable words of the valid rows: returns a dict with wmin, wmax, shift, direct (the plan alone
    answers), c (candidate count), cand (the candidate words in row order), pos (each rank's position among the SORTED candidates)
    and word (each rank's word, from the plan when direct, else from the sorted candidates)."""
    words = np.asarray(words, dtype=np.uint64)
    wmin, wmax = int(words.min()), int(words.max())
    span = wmax - wmin
    shift = digit_shift(span)
    if span == 0:
        return dict(wmin=wmin, wmax=wmax, shift=0, direct=True, c=0, cand=words[:0], pos=[0] * len(ranks), word=[wmin] * len(ranks))
    digit = ((words - np.uint64(wmin)) >> np.uint64(shift)).astype(np.int64)
    assert digit.max() < NBINS
    hist = np.bincount(digit, minlength=NBINS)
    pre = np.concatenate([[0], np.cumsum(hist)[:-1]])
    bins = [int(np.searchsorted(pre, r, side="right")) - 1 for r in ranks]
    offs = [r - int(pre[b]) for r, b in zip(ranks, bins)]
    wanted = np.zeros(NBINS, dtype=bool)
    wanted[bins] = True
    if shift == 0:
        return dict(wmin=wmin, wmax=wmax, shift=0, direct=True, c=0, cand=words[:0], pos=offs, word=[wmin + b for b in bins])
    chist = np.where(wanted, hist, 0)
    cpre = np.concatenate([[0], np.cumsum(chist)[:-1]])
    cand = words[wanted[digit]]
    pos = [int(cpre[b]) + o for b, o in zip(bins, offs)]
    srt = np.sort(cand)
    return dict(wmin=wmin, wmax=wmax, shift=shift, direct=False, c=int(chist.sum()), cand=cand, pos=pos,
                word=[int(srt[p]) for p in pos])


def stable_sorted(vals: np.ndarray) -> np.ndarray:
    """the valid values in the sort's order, ties (+-0, NaN payloads) in input order"""
    return vals[np.argsort(sortable_words(vals), kind="stable")]


def expected(sorted_vals: np.ndarray, qs, interp: str):
    """(elems (nq, 2), f64 (nq,)) of the quantiles of the sorted valid values"""
    n = len(sorted_vals)
    elems = np.zeros((len(qs), 2), dtype=sorted_vals.dtype)
    f64 = np.zeros(len(qs), dtype=np.float64)
    for j, q in enumerate(qs):
        ix = index(n, q)
        elems[j] = sorted_vals[ix[0]], sorted_vals[ix[1]]
        f64[j] = interpolate(interp, elems[j, 0], elems[j, 1], ix)
    return elems, f64
