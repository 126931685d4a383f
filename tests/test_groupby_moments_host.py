"""The checker of tests/test_gpu_groupby_moments.py, checked on the host: the exact reference reproduces the reference's golden
VARIANCE / STD vectors, the contract check rejects the one-pass formula sum x^2 - (sum x)^2 / c on the inputs that make it cancel
(even with correctly rounded sums) and accepts a plain two-pass with room to spare."""
import math

import numpy as np
import pytest

from oracle import cudf_oracle as orc
from tests import moments_cases as mc
from tests.golden import reference_vectors as gv


@pytest.mark.parametrize("case", [c for c in gv.GROUPBY if c["agg"] in ("var", "std")], ids=lambda c: c["name"])
def test_exact_m2_reproduces_the_golden_vectors(case):
    keys, km = gv.col(case["keys"], "int32", case.get("keys_valid"))
    vals, vm = gv.col(case["vals"], case.get("vals_dtype", "float64"), case.get("vals_valid"))
    km = np.ones(len(keys), bool) if km is None else km
    vm = np.ones(len(keys), bool) if vm is None else vm
    uniq = np.array(case["expect_keys"], np.int32)
    at = np.minimum(np.searchsorted(uniq, keys), len(uniq) - 1)
    labels = np.where(km & vm & (uniq[at] == keys), at, -1)
    m = np.array([int(v) for v in np.where(km & vm, vals, 0)], dtype=object)
    assert np.array_equal(np.asarray(m, np.float64)[km & vm], np.asarray(vals, np.float64)[km & vm])  # the golden values are integers
    m2, _, c = orc.exact_m2(m, 0, labels, len(uniq))
    ddof = case.get("ddof", 1)
    ev = np.array(case["expect_valid"], bool)
    np.testing.assert_array_equal(c - ddof > 0, ev)
    got = m2[ev] / (c[ev] - ddof)
    if case["agg"] == "std":
        got = np.sqrt(got)
    assert np.all(orc.ulp_diff(got, np.array(case["expect"], np.float64)[ev]) <= 1)


def _per_group(ds, fn):
    """fn(valid values of the group as float64) for every group of the reference without nulls, in its order"""
    ref = ds.reference(False)
    rows = np.argsort(ds.gid, kind="stable")
    bounds = np.searchsorted(ds.gid[rows], np.arange(ds.ngroups + 1))
    x = ds.x.astype(np.float64)
    return ref, np.array([fn(x[rows[bounds[g]:bounds[g + 1]]]) for g in ref["group"]])


def _one_pass(x):  # correctly rounded sums: better than any kernel delivers
    return orc.exact_sum(x * x) - orc.exact_sum(x) ** 2 / len(x) if np.isfinite(x).all() else np.nan


def _two_pass(x):
    if not np.isfinite(x).all():
        return np.nan
    d = x - math.fsum(x) / len(x)
    return math.fsum(d * d)


def _check_all(ref, m2, ddof):
    ok = np.ones(len(m2), bool)
    worst = mc.check(ref, "m2", m2, ok, what="m2")
    with np.errstate(invalid="ignore", divide="ignore"):
        var = m2 / np.maximum(ref["count"] - ddof, 1)
        mc.check(ref, "var", var, ref["count"] - ddof > 0, ddof, "var")
        mc.check(ref, "std", np.sqrt(var), ref["count"] - ddof > 0, ddof, "std")
    return worst


@pytest.mark.parametrize("families", [("const_",), ("centre_1e+08", "centre_-1e+08", "centre_1e+12")], ids=["constant", "large_mean"])
def test_the_one_pass_formula_fails_the_contract(families):
    ds = mc.Moments("float64", families=families)
    ref, m2 = _per_group(ds, _one_pass)
    with pytest.raises(AssertionError):
        mc.check(ref, "m2", m2, np.ones(len(m2), bool))
    if families == ("const_",):  # a negative M2 of a constant group: the negative VAR and the NaN STD are caught as such
        assert (m2 < 0).any()
        var = m2 / np.maximum(ref["count"] - 1, 1)
        with pytest.raises(AssertionError, match="negative var"):
            mc.check(ref, "var", var, ref["count"] > 1)
        with pytest.raises(AssertionError, match="std is NaN"), np.errstate(invalid="ignore"):
            mc.check(ref, "std", np.sqrt(var), ref["count"] > 1)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("ddof", [0, 1, 2])
def test_a_plain_two_pass_meets_the_contract_with_room(dtype, ddof):
    ds = mc.Moments(dtype)
    ref, m2 = _per_group(ds, _two_pass)
    assert _check_all(ref, m2, ddof) < 0.5


def test_reference_with_nulls_and_the_null_key_group():
    """the reference itself: counts against a plain count, the null-key group last, groups whose keys are all null absent"""
    ds = mc.Moments("float32")
    ref = ds.reference(True, null_group=True)
    kv, vv = ds.keys_valid, ds.values_valid
    assert ref["group"][-1] == -1 and ref["count"][-1] == int((~kv & vv).sum())
    for row in (0, 7, len(ref["group"]) - 2):
        g = ref["group"][row]
        assert ref["count"][row] == int((kv & vv & (ds.gid == g)).sum())
    assert set(ref["group"][:-1]) == set(np.unique(ds.gid[kv]))
    assert ref["nonfinite"].sum() == 4 and ds.reference(True)["m2"].shape[0] == len(ref["m2"]) - 1
