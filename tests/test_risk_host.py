"""What the GPU tests of the objective, the accuracy and the fairness statistics (test_gpu_risk.py) claim about their
inputs, pinned on a CPU: where every tie pattern of tests/risk_fixtures.py lays its tie group relative to the band
starts of the family it was built for, that the exact reference agrees with oracle/objective.py, and that every score
pattern has the ties and the counts it names."""
import math

import numpy as np
import pytest

import risk_fixtures as F
from oracle import objective, weights, zband

FAMS = F.BANDED + F.SMOOTH + ["erm"]
HOST_SIZES = [16, 17, 19, 1000, 4099]          # (70001 is built the same way; the GPU file runs it)


def _fam_n():
    return [(fam, n) for fam in FAMS for n in HOST_SIZES]


def test_band_starts_are_those_of_sigma():
    """the edges the patterns are built on: positions where sigma changes (oracle/zband.py: bands_of); every banded
    family has 2 to 5 bands at every size, first and last of two or more ranks - what the library's setup accepts"""
    for fam in F.BANDED:
        for n in F.SIZES:
            wf, args, _ = F.family(fam, n)
            starts = F.band_starts(wf, args, n)
            ref, values = zband.bands_of(weights.get_weights(wf, n, args)[0])
            assert starts == [int(s) for s in ref]
            assert 3 <= len(starts) <= 6 and starts[1] >= 2 and n - starts[-2] >= 2, (fam, n, starts)
            assert zband.clusters_of(ref, values) is not None, (fam, n)
            assert F.edges(wf, args, n) == [s - 1 for s in starts[1:-1]]
    assert F.band_starts("superquantile", [0.5], 16) == [0, 8, 16]           # the fractional weight equals the plateau's
    assert F.band_starts("superquantile", [0.5], 17) == [0, 8, 9, 17]
    assert F.band_starts("aorr_dc", [9, 1], 16) == [0, 2, 9, 10, 11, 16]
    assert F.band_starts("extremile", [2.0], 1000) == [0, 333, 666, 1000]    # nominal
    assert F.band_starts("erm", None, 19) == [0, 6, 12, 19]


@pytest.mark.parametrize("fam,n", _fam_n(), ids=[f"{f}-{n}" for f, n in _fam_n()])
def test_tie_groups_lie_where_their_names_say(fam, n):
    wf, args, _ = F.family(fam, n)
    starts, ed = F.band_starts(wf, args, n), F.edges(wf, args, n)
    for name, case in F.cases(n, wf, args):
        v = F.pattern(name, n, wf, args, seed=3, case=case)
        assert v.shape == (n,) and v.dtype == np.float64
        assert np.array_equal(v, F.pattern(name, n, wf, args, seed=3, case=case))
        lay = F.layout(name, n, wf, args, case)
        s = np.sort(v)
        if name in ("gaussian", "extremes"):
            assert lay is None and np.unique(v).size == n
        elif name == "ascending":
            assert np.all(v[1:] > v[:-1])
        elif name == "descending":
            assert np.all(v[1:] < v[:-1])
        elif name == "all_equal":
            assert np.all(v == 0.3) and lay == (0, n)
        elif name == "two_values":
            c = lay[1]
            assert np.all(s[:c] == F.TWO[0]) and np.all(s[c:] == F.TWO[1]) and 1 <= c <= n - 1
            start = starts[1 + case // 3]
            assert c == min(max(start + case % 3 - 1, 1), n - 1)       # the lower value's count: a band start, +- 1
        elif name == "dup33":
            vals, counts = np.unique(v, return_counts=True)
            assert vals.size == (n + 32) // 33 and np.all(counts[np.argsort(counts)][1:] == 33)
        elif name == "hinge_plateau":
            assert np.count_nonzero(v <= -1.0) == (9 * n) // 10 and np.count_nonzero(v == -1.0) >= 1
            assert np.count_nonzero(F.sample_losses(F.HINGE, v) == 0.0) == (9 * n) // 10
        else:
            a, b = lay
            e = ed[case // 2] if name == "signed_zeros" else (ed[case] if name != "span_all_edges" else None)
            if name == "signed_zeros":
                z = F.zero_split(n, wf, args, case)
                s = v[np.argsort(F.flip_keys(v), kind="stable")]       # key order: -0.0 before +0.0 (np.sort mixes them)
                assert F.group_of(v, a) == (a, z) and F.group_of(v, b - 1) == (z, b)
                assert np.all(np.signbit(s[a:z])) and not np.any(np.signbit(s[z:b])) and np.all(s[a:b] == 0.0)
                assert a <= e < b and (z == min(e + 3, b) if case % 2 == 0 else z == e + 1)
                assert np.all(s[:a] < 0.0) and np.all(s[b:] > 0.0)
                continue
            assert F.group_of(v, a) == (a, b), (name, case, F.group_of(v, a), (a, b))
            assert np.unique(s).size == n - (b - a) + 1                # no other ties
            if name == "span_one_edge":
                assert a == max(0, e - 3) and b == min(n, e + 6) and a <= e and b >= e + 2
            elif name == "ends_on_edge":
                assert b - 1 == e and a == max(0, e - 4)               # the group's last element IS the band's last rank
            elif name == "starts_after_edge":
                assert a == e + 1 and b == min(n, e + 6) and b > a     # begins at the next band's first rank
            else:
                assert a >= 1 and b <= n - 1                           # distinct values on both sides
                assert all(a <= x and x + 1 < b for x in ed)           # every edge and the rank behind it


def test_every_tie_pattern_reaches_every_edge():
    for fam in F.BANDED:
        for n in F.SIZES[:5]:
            wf, args, _ = F.family(fam, n)
            ne = len(F.edges(wf, args, n))
            assert [F.ncases(nm, n, wf, args) for nm in ("span_one_edge", "ends_on_edge", "starts_after_edge")] == [ne] * 3
            assert F.ncases("signed_zeros", n, wf, args) == 2 * ne and F.ncases("two_values", n, wf, args) == 3 * ne
            assert F.ncases("gaussian", n, wf, args) == 1


@pytest.mark.parametrize("fam", FAMS)
def test_risk_exact_equals_the_oracle_objective_on_gaussian(fam):
    for n in (17, 1000):
        wf, args, _ = F.family(fam, n)
        v = F.pattern("gaussian", n, wf, args, seed=1)
        sigma = weights.get_weights(wf, n, args)[0]
        for loss in F.losses_of(fam):
            got = F.risk_exact(wf, args, loss, v)
            if loss == F.SQ:                                           # oracle/objective.py knows the reference's two losses
                ref = float(np.dot(sigma, np.sort(np.maximum(1.0 + v, 0.0) ** 2)))
            else:
                ref = objective.objective_from_v(loss, sigma, v, np.zeros(1))
            assert abs(got - ref) <= 1e-14 * max(1.0, abs(ref)), (fam, n, loss, got, ref)
            r = np.where(np.arange(n) % 3 == 0, -1.0, 1.0)
            assert F.risk_exact(wf, args, loss, r * v, r=r) == got    # r * (r * v) = v exactly


@pytest.mark.parametrize("fam", FAMS)
def test_all_equal_signed_zeros_extremes(fam):
    for n in (16, 19, 1000):
        wf, args, _ = F.family(fam, n)
        sigma = weights.get_weights(wf, n, args)[0]
        for loss in F.losses_of(fam):
            l03 = float(F.sample_losses(loss, np.array([0.3]))[0])
            want = math.fsum(sigma * l03)
            got = F.risk_exact(wf, args, loss, F.pattern("all_equal", n, wf, args))
            assert abs(got - want) <= 1e-15 * want, (fam, n, loss)
            for case in range(F.ncases("signed_zeros", n, wf, args)):
                v = F.pattern("signed_zeros", n, wf, args, seed=2, case=case)
                assert np.count_nonzero(np.signbit(v) & (v == 0.0)) >= 1
                assert F.risk_exact(wf, args, loss, v) == F.risk_exact(wf, args, loss, np.where(v == 0.0, 0.0, v))
            v = F.pattern("extremes", n, wf, args, seed=2)
            assert sorted(v[np.isin(v, F.EXTREMES)]) == sorted(F.EXTREMES)
            assert np.all(np.isfinite(F.sample_losses(loss, v))) and math.isfinite(F.risk_exact(wf, args, loss, v))


@pytest.mark.parametrize("n", [17, 1000, 70001])
def test_scores_have_the_ties_and_counts_they_claim(n):
    for name in F.SCORES:
        x, y = F.scores(name, n, seed=1)
        assert x.shape == y.shape == (n,) and set(np.unique(y)) == {-1.0, 1.0}
        x2, y2 = F.scores(name, n, seed=1)
        assert np.array_equal(x, x2) and np.array_equal(y, y2)
        for t in F.THRESHOLDS:
            d = np.abs(x - F.logit(t))
            assert np.all((d >= F.GAP) | (x == 0.0))
        zeros = x == 0.0
        if name == "on_threshold":
            for neg in (False, True):
                for lab in (1.0, -1.0):
                    assert np.count_nonzero(zeros & (np.signbit(x) == neg) & (y == lab)) == F.ON_THRESHOLD
            assert np.all(F._probs(x[zeros]) == 0.5)
            # both zeros predict +1 at threshold 0.5: right under y = +1, wrong under y = -1
            pred = np.where(F._probs(x) >= 0.5, 1, -1)
            assert np.all(pred[zeros] == 1)
        else:
            assert not zeros.any()
        if name == "extreme":
            for val in (745.0, -745.0, 1e6, -1e6):
                assert sorted(y[x == val]) == [-1.0, 1.0]
        yk = F.relabel(y, seed=1)
        assert 0 < np.count_nonzero(yk != y) < n and set(np.unique(yk)) <= {-1.0, 1.0}
    g = {nm: F.groups(nm, n, seed=1) for nm in F.GROUPS}
    assert set(np.unique(g["binary"])) == {0.0, 1.0}
    assert set(np.unique(g["with_twos"])) == {0.0, 1.0, 2.0} and np.count_nonzero(g["with_twos"] == 2.0) == max(2, n // 50)
    assert np.all(g["no_group0"] == 1.0) and np.all(g["no_group1"] == 0.0)


def test_reference_statistics_on_a_hand_made_table():
    """accuracy_ref / fair_ref on eight rows whose counts can be read off"""
    xw = np.array([2.0, -2.0, 0.0, -0.0, 1.0, -1.0, 3.0, -3.0])
    y = np.array([1.0, 1.0, 1.0, -1.0, -1.0, -1.0, 1.0, -1.0])
    grp = np.array([0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 2.0])
    assert F.accuracy_ref(xw, y, 0.5, F.BCE) == 5 / 8                   # right: rows 0, 2, 5, 6, 7
    assert F.accuracy_ref(xw, y, 0.5, F.HINGE) == 4 / 8                 # the fraction of y = +1
    assert F.accuracy_ref(xw, y, 0.5, F.SQ) == F.accuracy_ref(xw, y, 0.5, F.BCE)
    SPD, DI, EOD, AOD, TI, FNRD = F.fair_ref(xw, y, grp, 0.5)
    # group 0: rows 0-3, predicted + = rows 0, 2, 3 -> 3/4; TP 2, FN 1, FP 1, TN 0.  group 1: rows 4-6, + = 4, 6 -> 2/3; TP 1, FN 0, FP 1, TN 1
    assert SPD == 2 / 3 - 3 / 4 and DI == (2 / 3) / (3 / 4)
    assert EOD == 1.0 - 2 / 3 and AOD == 0.5 * (0.5 - 1.0 + EOD) and FNRD == 0.0 - 1 / 3
    p = F._probs(xw)
    b = p - (y > 0) + 1.0
    mu = b.mean()
    assert abs(TI - np.mean(b / mu * np.log(b / mu))) <= 1e-15         # fair_metric.py:36-39 in its own form; row 7 included
    with np.errstate(all="ignore"):
        out = F.fair_ref(xw, y, np.zeros(8), 0.5)
    assert math.isnan(out[0]) and math.isnan(out[1]) and math.isnan(out[5]) and math.isfinite(out[4])
