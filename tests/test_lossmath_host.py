"""The loss-math reference of tests/lossmath_ref.py is certified (mpmath, exact rationals), the float64 restatements
the rest of the suite leans on (oracle/prox.py, tests/sqhinge_ref.py) are measured against it on inputs that reach the
edges of the arithmetic, and the designs of the PAV and EHRM device cases are shown to be valid.  CPU only.  Each
measurement prints its worst value (pytest -s)."""
from fractions import Fraction

import numpy as np
import pytest

import lossmath_ref as R
import sqhinge_ref
from oracle import prox as oprox

LD = R.LD


@pytest.fixture(scope="module")
def tab():
    sigma, rho, m = R.tables()
    return dict(sigma=sigma, rho=rho, m=m, x={loss: R.prox(loss, sigma, rho, m) for loss in R.LOSSES})


def test_tables_reach_the_edges(tab):
    sigma, rho, m = tab["sigma"], tab["rho"], tab["m"]
    ratio = sigma / rho
    assert m.size >= 4400 and np.all(np.abs(m) <= 1e15)
    assert ratio.max() >= 1e13 and ratio[ratio > 0].min() <= 1e-13 and np.count_nonzero(sigma == 0) >= 50
    assert np.all(np.log2(rho) == np.round(np.log2(rho))) and rho.min() == 2.0 ** -40 and rho.max() == 2.0 ** 20
    for v in (36.5, 37.5, 700.0, 745.2, 746.0, 1e6, 1e15, 1e-300, 0.0):
        assert np.any(m == v) and np.any(m == -v)
    e = R.edge_m()
    assert e.size == 429 and all(np.any(e == v) for v in R.EDGE_LIST)
    assert np.array_equal(R.edge_m(3)[:3], e[:3]) and R.edge_m(1000).size == 1000


def test_bce_root_is_certified_by_mpmath(tab):
    """mpmath at 50 digits, on the whole grid and 600 of the random points: g(x - delta) <= 0 <= g(x + delta) with
    delta = 2^-60 scale.  g is increasing, so the exact root lies within delta of the longdouble one: the statement
    "agrees with a 50-digit solve to 2^-60 scale" without trusting a second root finder."""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    sigma, rho, m, x = tab["sigma"], tab["rho"], tab["m"], tab["x"][R.BCE]
    n_grid = R.grid()[0].size
    idx = list(range(n_grid)) + list(range(n_grid, n_grid + 600))
    sc = R.scale(x, m)

    def to_mp(v):
        q = R.ld_to_fraction(v)
        return mp.mpf(q.numerator) / mp.mpf(q.denominator)

    def g(s, r, mm, t):
        sig = 1 / (1 + mp.exp(-t)) if t > -10000 else mp.exp(t)      # (1 + exp(-t) is exp(-t) to 4000 digits there)
        return s * sig + r * (t - mm)

    bad = []
    for i in idx:
        s, r, mm, xi = mp.mpf(float(sigma[i])), mp.mpf(float(rho[i])), mp.mpf(float(m[i])), to_mp(x[i])
        delta = to_mp(sc[i]) * mp.mpf(2) ** -60
        if not (g(s, r, mm, xi - delta) <= 0 <= g(s, r, mm, xi + delta)):
            bad.append((i, float(sigma[i]), float(rho[i]), float(m[i]), float(x[i])))
    assert not bad, bad[:5]
    assert np.all(x[sigma == 0] == m[sigma == 0])


@pytest.mark.parametrize("loss", [R.HINGE, R.SQ])
def test_closed_forms_against_exact_rationals(tab, loss):
    """longdouble closed forms against fractions.Fraction on every table entry: equal once the exact value is rounded
    to the reference's own precision (two longdouble operations: 2^-62 scale)"""
    sigma, rho, m, x = tab["sigma"], tab["rho"], tab["m"], tab["x"][loss]
    sc = R.scale_of(loss, x, sigma, rho, m)
    worst = 0.0
    for i in range(m.size):
        q = R.prox_fraction(loss, sigma[i], rho[i], m[i])
        err = abs(R.ld_to_fraction(x[i]) - q)
        worst = max(worst, float(err / Fraction(float(sc[i]))))
        assert abs(R.fraction_to_ld(q) - x[i]) <= LD(2.0 ** -62) * sc[i], (loss, i)
    print(f"lossmath-host closed form {loss}: worst |longdouble - exact| / scale = {worst:.2e}")
    assert worst <= 2.0 ** -62


def _oracle(loss, sigma, rho, m):
    out = np.empty(m.size)
    for r in np.unique(rho):
        k = rho == r
        out[k] = sqhinge_ref.prox(sigma[k], r, m[k]) if loss == R.SQ else oprox.prox_exact(loss, sigma[k], r, m[k])
    return out


@pytest.mark.parametrize("loss", R.LOSSES)
def test_oracle_prox_against_the_reference(tab, loss):
    """the float64 restatements every other prox test compares the device with (oracle/prox.py: prox_exact,
    tests/sqhinge_ref.py: prox), against a reference that shares neither their algorithm nor their precision"""
    sigma, rho, m, x = tab["sigma"], tab["rho"], tab["m"], tab["x"][loss]
    got = _oracle(loss, sigma, rho, m)
    e = R.err_units(got, x, R.scale_of(loss, x, sigma, rho, m))
    k = int(np.argmax(e))
    print(f"lossmath-host oracle {loss}: worst error {e[k]:.3f} eps scale (bar {R.BAR_ORACLE[loss]}) at sigma={sigma[k]:.3e} "
          f"rho=2^{int(np.log2(rho[k]))} m={m[k]:.17g}")
    assert np.all(np.isfinite(got))
    assert e[k] <= R.BAR_ORACLE[loss]
    zero = sigma == 0
    assert np.array_equal(got[zero], m[zero])


def test_losses_against_mpmath():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    for v in R.EDGE_LIST + [0.3, -0.3, 20.0, -20.0]:
        t = mp.mpf(v)
        sp = max(t, 0) + mp.log1p(mp.exp(-abs(t)))
        sg = 1 / (1 + mp.exp(-t))
        for got, ref in ((R.softplus(v), sp), (R.sigmoid(v), sg)):
            q = R.ld_to_fraction(got)
            assert abs(mp.mpf(q.numerator) / mp.mpf(q.denominator) - ref) <= mp.mpf(2) ** -61 * abs(ref) + mp.mpf(10) ** -4900   # (underflow)
    v = np.array([-3.0, -1.0, -0.5, 2.0])
    assert np.array_equal(R.sample_loss(R.HINGE, v), [0, 0, 0.5, 3]) and np.array_equal(R.sample_loss(R.SQ, v), [0, 0, 0.25, 9])


# ------------------------------------------------------------------------------------------------ designs of the device cases
def _pav_cases():
    out = [("separate", None), ("segments", None)] + [("one_block", n) for n in R.PAV_ONE_BLOCK_N]
    return out


@pytest.mark.parametrize("kind,n", _pav_cases())
def test_pav_designs_are_valid(kind, n):
    """dyadic inputs whose prefix sums are exact; inside a segment the element values DEcrease (equal m, increasing
    sigma: everything pools), across segments the block values increase by far more than the device's bar, so the
    exact PAV solution is one block per segment"""
    sigma, m, seg = R.pav_design(kind, n)
    assert seg.sum() == m.size and np.all(np.diff(m) >= 0)
    assert R.prefix_sums_exact(sigma) and R.prefix_sums_exact(m) and R.prefix_sums_exact(np.abs(m))
    ends = np.cumsum(seg)
    if kind == "segments":
        assert any(a < 2048 < b for a, b in zip(ends - seg, ends))
        for loss in (R.BCE, R.SQ):         # the long segments pool strictly: their merge count is known
            assert all(np.all(R.pav_strict_segments(loss, sigma, rho, m, seg)[3:]) for rho in R.PAV_RHO)
    if kind == "separate":
        assert m.size > 2048 + 64
    if kind == "one_block" and n != 64:
        assert all(R.pav_strict_segments(R.BCE, sigma, rho, m, seg)[0] for rho in R.PAV_RHO)
    for rho in R.PAV_RHO:
        for loss in R.LOSSES:
            pos, x, sc = R.pav_reference(loss, sigma, rho, m, seg)
            gap = np.diff(x)
            need = 4 * R.BAR_PAV * R.EPS * np.maximum(sc[ends[:-1] - 1], sc[ends[:-1]])
            strict = (kind != "one_block") and (loss != R.HINGE)
            if strict:          # (the hinge runs design "one_block" only)
                assert np.all(gap > need), (kind, loss, rho, float(np.min(gap / need)))
            for a, b in zip(ends - seg, ends):
                if b - a > 1:
                    el = R.prox(loss, sigma[a:b], LD(rho), m[a:b])
                    assert np.all(np.diff(el) <= 0), (kind, loss, rho)       # every neighbour violates: one block
    if kind != "one_block" or n >= 2047:
        assert float(np.mean(sigma[-seg[-1]:])) / min(R.PAV_RHO) >= 5e5     # a pooled sigma / rho of about 1e6


@pytest.mark.parametrize("B", R.EHRM_B)
@pytest.mark.parametrize("rho", R.EHRM_RHO)
def test_ehrm_designs_are_valid(B, rho):
    m = R.ehrm_design(B, rho)
    sa, sb = R.ehrm_weights()
    assert m.size == R.EHRM_N and np.all(np.diff(m) >= 0)
    ta, tb = R.ehrm_thresholds(B, rho)
    hit = 0
    for i0, i1 in R.TH:
        for t in (ta, tb):
            rel = (m[i0:i1] - t[i0:i1]) / np.abs(t[i0:i1])
            if np.all(np.abs(rel) <= 1.5e-12):
                hit += 1
                assert np.any(rel > 0) and np.any(rel < 0) and np.any(rel == 0)
    assert hit == 2
    for v in R.EHRM_EDGE:
        if v not in (0.0, 1e-300, -1e-300):
            assert np.any(m == v), v
    ref = R.ehrm_reference(B, rho, m)
    f1, f2 = ref["f1"], ref["f2"]
    sep = float(abs(f1 - f2) / (abs(f1) + abs(f2)))
    print(f"lossmath-host ehrm B={B} rho=2^{int(np.log2(rho))}: f1={float(f1):.12g} f2={float(f2):.12g} separation {sep:.2e}")
    assert sep > 1e-9
    d = np.abs(np.asarray(ref["pa"] - m, dtype=np.float64))
    if rho == max(R.EHRM_RHO):
        assert np.mean(d < 1e-3) > 0.9 and d[m == -700.0][0] < 1e-3       # the expansion, m = -700 included
    else:
        assert np.mean(d > 1e-3) > 0.5                                     # softplus itself
    # the monotone case: neither branch pools, with room for the device's rounding
    mm = R.ehrm_monotone(B)
    for s in (sa, sb):
        x = R.prox_bce(s, R.EHRM_MONO_RHO, mm)
        assert np.all(np.diff(x) > 4 * R.BAR[R.BCE] * R.EPS * R.scale(x, mm)[1:])


def test_ehrm_close_call_is_a_close_call():
    B, rho, m = R.ehrm_close_call()
    assert m.size == R.EHRM_N and np.all(np.diff(m) > 0)
    ref = R.ehrm_reference(B, rho, m)
    sep = float((ref["f2"] - ref["f1"]) / (ref["f1"] + ref["f2"]))
    print(f"lossmath-host ehrm close call: f1={float(ref['f1']):.15g} f2={float(ref['f2']):.15g} (f2 - f1) / (f1 + f2) = {sep:.3e}")
    assert ref["branch"] == 0 and 1e-9 < sep < 2e-8
    d = np.abs(np.asarray(ref["pa"] - m, dtype=np.float64))[m < B]
    assert np.mean(d > 1e-3) == 1.0 and np.mean(d <= 1e-1) > 0.6   # softplus itself today; an expansion used out to 0.1 would take most of f1
