"""Row weights (sample_weight / class_weight, include/rbl.h: rbl_set_row_weights), the part that needs no GPU: the
weighted CPU reference tests/weighted_ref.py against oracle.admm (c == 1: the same bits) and against the problem it
claims to solve (integer weights = repeated rows), _solver.resolve_row_weights with every refusal raised before any
device call, and the new symbols in header, library and binding."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from oracle import admm as oracle_admm
from oracle import problems
from oracle.prox import sigmoid
import weighted_ref


def _pkg():
    import admm_for_rank_based_loss_amd as rbl
    return rbl


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("loss", ["binary_cross_entropy", "hinge"])
@pytest.mark.parametrize("reg", ["l1_reg", "l2_reg"])
def test_unit_weights_are_the_oracle_bit_for_bit(loss, reg):
    """c == 1: sigma_i = 1.0 * (1 / n) has the bits of the oracle's 1 / n, so 25 iterations return admm_solve's w with
    difference exactly 0"""
    X, y = problems.make_problem(200, 12, seed=5)
    kw = {reg: 0.01}
    ref = oracle_admm.admm_solve(X, y, weight_function="erm", loss=loss, max_iter=25, tol=0.0, mode="exact", **kw)
    got = weighted_ref.admm(X, y, np.ones(200), loss, max_iter=25, tol=0.0, **kw)
    diff = float(np.max(np.abs(got.w - ref.w)))
    print(f"weighted_ref c=1 {loss} {reg}: max |dw| = {diff!r}")
    assert diff == 0.0
    assert np.array_equal(got.z, ref.z) and np.array_equal(got.lam, ref.lam) and got.rho == ref.rho


def test_integer_weights_solve_the_repeated_rows_problem():
    """BCE with l2_reg = 0.05, n = 240, d = 8, integer c in {0..3}: the weighted run against the unweighted run on the
    rows repeated c_i times with l2_reg * n / sum(c) (the same minimiser: F_c = (sum(c) / n) F_rep).  F_c is strongly
    convex with modulus l2_reg, so for any two points ||w_a - w_b|| <= (||grad F_c(w_a)|| + ||grad F_c(w_b)||) / l2_reg
    with grad F_c(w) = D^T (c * sigmoid(D w)) / n + l2_reg w.  Both gradient norms must also be below tol * ||D||_2, so
    that the bound cannot pass vacuously.  (Seen: 228 and 160 iterations, distance 1.2e-9 under a bound of 9.4e-9,
    gradient norms 4.5e-10 and 2.1e-11.)  Only BCE with l2 is used: with hinge or l1 the stop rule fires far from the
    minimiser at this size, which proves nothing."""
    n, d, l2, tol = 240, 8, 0.05, 1e-9
    X, y = problems.make_problem(n, d, seed=11)
    rng = np.random.default_rng(3)
    c = rng.integers(0, 4, size=n).astype(np.float64)
    assert 0.15 < np.mean(c == 0) < 0.35
    a = weighted_ref.admm(X, y, c, "binary_cross_entropy", l2_reg=l2, max_iter=5000, tol=tol)
    rep = np.repeat(np.arange(n), c.astype(int))
    b = oracle_admm.admm_solve(X[rep], y[rep], weight_function="erm", loss="binary_cross_entropy",
                               l2_reg=l2 * n / float(np.sum(c)), max_iter=5000, tol=tol, mode="exact", store=False)
    assert a.converged and b.converged
    D = -np.asarray(y).reshape(-1, 1) * X

    def grad(w):
        return D.T @ (c * sigmoid(D @ w)) / n + l2 * w

    ga, gb = float(np.linalg.norm(grad(a.w))), float(np.linalg.norm(grad(b.w)))
    dist, bound = float(np.linalg.norm(a.w - b.w)), (ga + gb) / l2
    print(f"weighted_ref repeated rows: iters {a.iters} / {b.iters}, ||dw|| = {dist:.3e}, bound {bound:.3e}, "
          f"gradient norms {ga:.3e} / {gb:.3e}")
    spec = float(np.linalg.norm(D, 2))
    assert ga < tol * spec and gb < tol * spec, (ga, gb, tol * spec)
    assert dist <= bound, (dist, bound)


# ------------------------------------------------------------------------------------------------ resolve_row_weights
def test_resolve_balanced_dict_and_product():
    S = _pkg()._solver
    y = np.array([1.0] * 30 + [-1.0] * 10)                     # a 3 : 1 split
    assert S.resolve_row_weights(y, None, None) is None
    c = S.resolve_row_weights(y, None, "balanced")
    assert c.dtype == np.float64 and c.shape == (40,)
    assert np.array_equal(c[:30], np.full(30, 40 / (2.0 * 30))) and np.array_equal(c[30:], np.full(10, 40 / (2.0 * 10)))
    assert math_close(float(np.sum(c)), 40.0)                  # balanced weights keep the total
    c = S.resolve_row_weights(y, None, {1: 0.5, -1: 3.0})
    assert np.array_equal(c, np.where(y > 0, 0.5, 3.0))
    sw = np.arange(40, dtype=np.float64)
    c = S.resolve_row_weights(y, sw, {1: 0.5, -1: 3.0})
    assert np.array_equal(c, np.where(y > 0, 0.5, 3.0) * sw)
    c = S.resolve_row_weights(y, sw, "balanced")
    assert np.array_equal(c, np.where(y > 0, 40 / 60.0, 2.0) * sw)
    c = S.resolve_row_weights(y, sw.astype(np.float32), None)
    assert c.dtype == np.float64 and np.array_equal(c, sw)


def math_close(a, b):
    return abs(a - b) <= 1e-12 * abs(b)


BAD = [
    ("wrong length", dict(sample_weight=np.ones(39)), "39 entries for 40 rows"),
    ("nan", dict(sample_weight=np.where(np.arange(40) == 7, np.nan, 1.0)), "row 7"),
    ("inf", dict(sample_weight=np.where(np.arange(40) == 5, np.inf, 1.0)), "row 5"),
    ("negative", dict(sample_weight=np.where(np.arange(40) == 9, -0.5, 1.0)), "row 9"),
    ("all zero", dict(sample_weight=np.zeros(40)), "all 40 weights are zero"),
    ("all zero by product", dict(sample_weight=np.where(np.arange(40) < 30, 0.0, 1.0), class_weight={1: 1.0, -1: 0.0}),
     "weights are zero"),
    ("unknown word", dict(class_weight="balance"), "balanced"),
    ("dict keys", dict(class_weight={1: 1.0, 0: 2.0}), "keys +1 and -1"),
    ("dict value", dict(class_weight={1: 1.0, -1: -2.0}), "class_weight[-1]"),
    ("rank-weighted family", dict(sample_weight=np.ones(40), weight_function="superquantile"), "PAV z-step does not apply"),
    ("rank-weighted family, class_weight", dict(class_weight="balanced", weight_function="aorr"), "PAV z-step does not apply"),
]


@pytest.mark.parametrize("name,kw,msg", BAD, ids=[b[0] for b in BAD])
def test_resolve_refusals(name, kw, msg):
    S = _pkg()._solver
    y = np.array([1.0] * 30 + [-1.0] * 10)
    with pytest.raises(ValueError) as e:
        S.resolve_row_weights(y, kw.get("sample_weight"), kw.get("class_weight"), kw.get("weight_function", "erm"))
    assert msg in str(e.value), str(e.value)


def test_refusals_come_before_any_device_call(monkeypatch):
    """a bad sample_weight or a rank-weighted family fails in the constructors before a handle exists: the Solver class is
    replaced by one that must never be built"""
    rbl = _pkg()
    X, y = problems.make_problem(40, 5, seed=1)

    class NoDevice:
        def __init__(self, *a, **k):
            raise AssertionError("a device handle was created before the row weights were checked")

    monkeypatch.setattr(rbl._solver, "Solver", NoDevice)
    bad = np.ones(40)
    bad[3] = -1.0
    with pytest.raises(ValueError, match="row 3"):
        rbl.ADMMmethod(X, y, l2_reg=0.1, sample_weight=bad)
    with pytest.raises(ValueError, match="PAV z-step does not apply"):
        rbl.ADMMmethod(X, y, weight_function="superquantile", args=[0.5], l2_reg=0.1, sample_weight=np.ones(40))
    with pytest.raises(ValueError, match="row 3"):
        rbl.smoothADMMmethod(X, y, l1_reg=0.1, sample_weight=bad)
    with pytest.raises(ValueError, match="row 3"):
        rbl.rankbasedObjective(X, y, sample_weight=bad)
    with pytest.raises(ValueError, match="problem 1: .*row 3"):
        rbl.ADMMgroup(X, y, [dict(l2_reg=0.1), dict(l2_reg=0.1, sample_weight=bad)])
    with pytest.raises(ValueError, match="problem 0: .*row 3"):
        rbl.OneVsRest(X, np.arange(40) % 3, l2_reg=0.1, sample_weight=bad)


# ------------------------------------------------------------------------------------------------ the symbols
def test_symbols_are_declared_exported_and_bound():
    rbl = _pkg()
    header = open(os.path.join(ROOT, "include", "rbl.h")).read()
    declared = set(re.findall(r"\b(rbl_[A-Za-z0-9_]+)\s*\(", header))
    lib = rbl._lib.load()
    for name in ("rbl_set_row_weights", "rbl_get_row_weights", "rbl_k_sweep_erm_w"):
        assert name in declared and name in rbl._lib.SIGNATURES and hasattr(lib, name), name
    assert len(rbl._lib.SIGNATURES["rbl_k_sweep_erm_w"][1]) == len(rbl._lib.SIGNATURES["rbl_k_sweep_erm"][1])
    assert callable(rbl._lib.k_sweep_erm_w)
    assert callable(rbl._solver.Solver.set_row_weights) and callable(rbl._solver.Solver.get_row_weights)
    assert "#define RBL_VERSION 106" in header and lib.rbl_version() == 106
