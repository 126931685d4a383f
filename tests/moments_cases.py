"""Inputs, exact reference and contract check of the groupby VARIANCE / STD / M2 tests (tests/test_gpu_groupby_moments.py on the
device, tests/test_groupby_moments_host.py for the check itself).

Every value is x = m * 2^-q with an integer |m| < 2^53 (for float32 columns: exactly a float32), so the exact moments come from
Python integers (oracle exact_m2).  The contract, with u = 2^-53, M2* the exact sum (x - mean)^2 and S2* the exact sum x^2 of a
group's valid values, both rounded once to float64:

  |M2 - M2*| <= 16u * M2* + 64u^2 * S2*,  M2 >= 0;
  VAR = M2 / (c - ddof) and STD = sqrt(VAR) within 4 further ulps of the same function of an M2 inside that interval, VAR >= 0,
  STD never NaN for finite values;  a group holding a NaN or an infinity gives NaN (valid) for all three;
  VAR / STD null where c - ddof <= 0, M2 valid everywhere (0 for a group without a valid value).

Centring on the computed mean m = mu + e gives sum (x - m)^2 = M2* + c e^2 exactly; a mean from a 1-ulp sum has |e| <= 3u |mu|,
so c e^2 <= 9 u^2 S2*; the roundings of d, d^2 and a 1-ulp sum of non-negative terms add at most 6u relative: 16 over 6, 64 over 9.
"""
import math

import numpy as np

from oracle import cudf_oracle as orc

U = 2.0 ** -53
COUNTS = (1, 2, 3, 7, 63, 64, 65, 1000, 4095, 4096, 4097)  # both sides of the wave, the tile and the scan chunk
LONG_GROUP = 50_021                                        # one group across many tiles and scan chunks


def _constant(x, q):
    m = int(math.ldexp(float(x), q))
    return lambda rng, c: np.full(c, m, np.int64)


def _centred(centre, q, spread):
    c0 = int(math.ldexp(float(centre), q))
    return lambda rng, c: c0 + rng.integers(-spread, spread + 1, c)


def _mean_zero(rng, c):  # magnitudes over 40 binades, random signs
    return rng.integers(1, 4096, c) * (1 << rng.integers(0, 41, c)) * rng.choice([-1, 1], c)


# (family, q, generator of m)
FAMILIES = {
    "float64": [("const_0.1", 50, _constant(0.1, 50)), ("const_1/3", 50, _constant(1 / 3, 50)),
                ("const_1e6+0.1", 30, _constant(1e6 + 0.1, 30)), ("const_123456.789", 33, _constant(123456.789, 33)),
                ("const_-2.5e-7", 70, _constant(-2.5e-7, 70))] +
               [(f"centre_{k:g}_spread_{s}", q, _centred(k, q, s)) for k, q in ((1e4, 20), (1e8, 20), (-1e8, 20), (1e12, 10))
                for s in (1, 1000, 1 << 20)] +
               [("mean_zero_40_binades", 30, _mean_zero)],
    "float32": [("const_0.1f", 27, _constant(np.float32(0.1), 27)), ("const_1/3f", 25, _constant(np.float32(1 / 3), 25)),
                ("centre_1000_spread_64", 10, _centred(1000, 10, 64)), ("centre_0_spread_64", 10, _centred(0, 10, 64))],
}
LONG_FAMILY = {"float64": "centre_1e+08_spread_1000", "float32": "centre_1000_spread_64"}
NON_FINITE = {"one_nan": [np.nan], "one_+inf": [np.inf], "+inf_and_-inf": [np.inf, -np.inf], "nan_only": [np.nan] * 3}


class Moments:
    """x: the values; m, q: their integers and exponents (m = 0 under a non-finite value); gid: the group of every row;
    special: the rows holding a NaN or an infinity; family: the name of every group.  families: only the families whose name
    starts with one of these, and no non-finite groups."""

    def __init__(self, dtype, seed=2024, families=None):
        rng = np.random.default_rng(seed)
        fams = [f for f in FAMILIES[dtype] if families is None or f[0].startswith(tuple(families))]
        ms, qs, gids, self.family = [], [], [], []

        def group(name, q, m):
            gids.append(np.full(len(m), len(self.family), np.int64))
            ms.append(np.asarray(m, np.int64))
            qs.append(np.full(len(m), q, np.int64))
            self.family.append(name)

        for name, q, gen in fams:
            for c in COUNTS + ((LONG_GROUP,) if name == LONG_FAMILY[dtype] else ()):
                group(name, q, gen(rng, c))
        first_special = len(self.family)
        if families is None:  # the finite rows of the non-finite groups: a family with a large mean
            name, q, gen = next(f for f in fams if f[0].startswith("centre"))
            for what, put in NON_FINITE.items():
                group(what, q, gen(rng, 3 if what == "nan_only" else 65))
        self.m, self.q, self.gid = np.concatenate(ms), np.concatenate(qs), np.concatenate(gids)
        self.x = np.ldexp(self.m.astype(np.float64), -self.q).astype(dtype)
        # every value is exactly its integer: |m| < 2^53, and the column's type holds m * 2^-q
        assert np.all(np.abs(self.m) < 2**53)
        assert np.array_equal(np.ldexp(self.x.astype(np.float64), self.q), self.m.astype(np.float64))
        self.special = np.zeros(len(self.x), bool)
        for g in range(first_special, len(self.family)):
            put = NON_FINITE[self.family[g]]
            rows = np.nonzero(self.gid == g)[0][-len(put):]
            self.x[rows] = put
            self.special[rows] = True
        self.m[self.special] = 0
        order = rng.permutation(len(self.x))  # shuffled keys
        self.m, self.q, self.gid, self.x, self.special = self.m[order], self.q[order], self.gid[order], self.x[order], self.special[order]
        self.n, self.ngroups = len(self.x), len(self.family)
        self.key_of_group = rng.permutation(self.ngroups).astype(np.int64)  # dense ids from zero, in no order of the families
        # 5 % null keys and 15 % null values; the rows holding a NaN / infinity stay valid so that their groups are what they say
        self.keys_valid = (rng.random(self.n) >= 0.05) | self.special
        self.values_valid = (rng.random(self.n) >= 0.15) | self.special
        self._refs = {}

    def keys(self, dtype=np.int64, scale=1, offset=0):
        return (self.key_of_group[self.gid] * scale + offset).astype(dtype)

    def values(self, nulls):
        """the column; with nulls, a NaN / a huge number lies under every null value"""
        if not nulls:
            return self.x
        x = self.x.copy()
        hidden = np.nonzero(~self.values_valid)[0]
        x[hidden[::2]], x[hidden[1::2]] = np.nan, 3e30
        return x

    def reference(self, nulls, null_group=False):
        """exact moments of the groups in ascending key order (null_group: the rows with a null key are one more group, last):
        dict(group = the group of self.family behind every result row (-1: the null group), count, m2, s2, nonfinite)"""
        if (nulls, null_group) in self._refs:
            return self._refs[nulls, null_group]
        kv = self.keys_valid if nulls else np.ones(self.n, bool)
        vv = self.values_valid if nulls else np.ones(self.n, bool)
        key = self.key_of_group[self.gid]
        present = np.unique(key[kv])                                       # ascending keys
        row_of_key = np.full(self.ngroups, -1, np.int64)
        row_of_key[present] = np.arange(len(present))
        extra = 1 if null_group and not kv.all() else 0
        g = len(present) + extra
        labels = np.where(kv, row_of_key[key], g - 1 if extra else -1)
        m2, s2, _ = orc.exact_m2(self.m, self.q, np.where(vv & ~self.special, labels, -1), g)
        counted = vv & (labels >= 0)
        ref = dict(group=np.concatenate([np.argsort(self.key_of_group)[present], np.full(extra, -1)]),
                   count=np.bincount(labels[counted], minlength=g), m2=m2, s2=s2,
                   nonfinite=np.bincount(labels[counted & self.special], minlength=g) > 0)
        self._refs[nulls, null_group] = ref
        return ref


def _step(x, k):
    """k ulps up (down for k < 0) from the non-negative doubles x, not below 0"""
    return np.maximum(np.asarray(x, np.float64).view(np.int64) + k, 0).view(np.float64)


def check(ref, kind, got, got_valid, ddof=1, what=""):
    """assert the contract of this file's docstring for kind in ("m2", "var", "std"); returns the largest |M2 - M2*| / tolerance
    (kind "m2") or 0"""
    got, got_valid = np.asarray(got, np.float64), np.asarray(got_valid, bool)
    c, m2, s2, bad = ref["count"], ref["m2"], ref["s2"], ref["nonfinite"]
    assert got.shape == m2.shape, f"{what}: {got.shape[0]} groups, expected {m2.shape[0]}"
    want_valid = np.ones(len(c), bool) if kind == "m2" else c - ddof > 0
    np.testing.assert_array_equal(got_valid, want_valid, err_msg=f"{what}: validity of {kind}")
    assert np.isnan(got[bad & want_valid]).all(), f"{what}: {kind} of a group holding a NaN / an infinity must be NaN"
    fin = want_valid & ~bad
    tol = (16 * U * m2 + 64 * U * U * s2)[fin]
    g, m2, den = got[fin], m2[fin], np.maximum(c[fin] - ddof, 1).astype(np.float64)
    assert not np.isnan(g).any(), f"{what}: {kind} is NaN for finite values in {int(np.isnan(g).sum())} of {len(g)} groups"
    assert (g >= 0).all(), f"{what}: negative {kind} in {int((g < 0).sum())} of {len(g)} groups, e.g. {g[g < 0][:3]}"
    if kind == "m2":
        err = np.abs(g - m2)
        ratio = np.divide(err, tol, out=np.where(err > 0, np.inf, 0.0), where=tol > 0)
        over = err > tol
        assert not over.any(), (f"{what}: M2 outside 16u M2* + 64u^2 S2* in {int(over.sum())} of {len(g)} groups, worst "
                                f"{ratio.max():.3g} x the tolerance (result row {int(np.nonzero(fin)[0][np.argmax(ratio)])})")
        return float(ratio.max()) if len(ratio) else 0.0
    lo, hi = np.maximum(m2 - tol, 0.0) / den, (m2 + tol) / den
    if kind == "std":
        lo, hi = np.sqrt(lo), np.sqrt(hi)
    over = (g < _step(lo, -4)) | (g > _step(hi, 4))
    assert not over.any(), f"{what}: {kind} more than 4 ulps outside the image of the M2 interval in {int(over.sum())} of {len(g)} groups"
    return 0.0
