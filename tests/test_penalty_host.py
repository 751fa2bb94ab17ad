"""Per-coordinate penalties without a GPU: the NumPy reference of the generalised w-step (tests/penalty_ref.py) meets its
own optimality conditions and reduces to the oracle's lasso and ridge, and the Python layer rejects bad weight vectors
on the host, before any device call."""
import numpy as np
import pytest

from penalty_ref import enet_gram_exact, enet_kkt_residual


def _problem(n, d, seed, collinear=False):
    rng = np.random.default_rng(seed)
    D = rng.standard_normal((n, d))
    if collinear:
        D[:, 5] = D[:, 3]                      # exactly collinear pair
    G = D.T @ D
    q = D.T @ rng.standard_normal(n)
    return rng, G, q


@pytest.mark.parametrize("n,d", [(40, 12), (200, 30)])
def test_reference_meets_its_kkt_conditions(n, d):
    rng, G, q = _problem(n, d, seed=n + d)
    qm = np.max(np.abs(q))
    bar = 1e-10 * max(1.0, qm)
    rho = 0.7
    cases = []
    l1 = 2 * rho * 0.3 * qm * rng.uniform(0.5, 2.0, d)
    l2 = rho * rng.uniform(0.0, 2.0, d)
    cases.append((l1, l2))                                     # elastic net, random factors
    l1z, l2z = l1.copy(), l2.copy()
    l1z[[1, 4]] = 0.0                                          # zero-penalty (free) coordinates
    l2z[1] = 0.0
    cases.append((l1z, l2z))
    cases.append((np.zeros(d), l2 + 0.1))                      # no l1 at all
    for a, b in cases:
        w = enet_gram_exact(G, q, rho, a, b, np.zeros(d))
        assert enet_kkt_residual(G, q, rho, a, b, w) <= bar
    # exactly collinear columns with b > 0: strictly convex, the minimiser is unique - two different starts agree
    rng, G, q = _problem(n, d, seed=7 * n + d, collinear=True)
    qm = np.max(np.abs(q))
    a = np.full(d, 2 * rho * 0.2 * qm)
    b = np.full(d, rho * 0.5)
    w1 = enet_gram_exact(G, q, rho, a, b, np.zeros(d))
    w2 = enet_gram_exact(G, q, rho, a, b, rng.standard_normal(d))
    assert enet_kkt_residual(G, q, rho, a, b, w1) <= 1e-10 * max(1.0, qm)
    assert np.max(np.abs(w1 - w2)) <= 1e-10 * max(1.0, np.max(np.abs(w1)))
    assert abs(w1[3] - w1[5]) <= 1e-10 * max(1.0, np.max(np.abs(w1)))      # symmetric columns, symmetric penalty


@pytest.mark.parametrize("n,d", [(40, 12), (200, 30)])
def test_reference_reduces_to_the_oracle(n, d):
    from oracle import wstep
    rng, G, q = _problem(n, d, seed=3 * n + d)
    rho, reg = 0.4, 0.5 * np.max(np.abs(q))
    w = enet_gram_exact(G, q, rho, np.full(d, reg), None, np.zeros(d))
    ref, _ = wstep.lasso_gram_exact(G, q, reg / (2 * rho), np.zeros(d))
    assert np.max(np.abs(w - ref)) <= 1e-10 * max(1.0, np.max(np.abs(ref)))
    w = enet_gram_exact(G, q, rho, None, np.full(d, reg), np.zeros(d))
    ref = wstep.ridge_gram_exact(G, q, rho, reg)
    assert np.max(np.abs(w - ref)) <= 1e-10 * max(1.0, np.max(np.abs(ref)))


def test_weights_are_validated_on_the_host():
    import admm_for_rank_based_loss_amd as R
    rng = np.random.default_rng(0)
    X = rng.standard_normal((20, 5))
    y = np.where(rng.random(20) < 0.5, 1.0, -1.0)
    with pytest.raises(ValueError, match="l1_weights: has 4 entries for 5"):
        R.ADMMmethod(X, y, l1_weights=np.ones(4))
    with pytest.raises(ValueError, match="l2_weights: entries must be >= 0"):
        R.ADMMmethod(X, y, l1_reg=0.1, l2_weights=[1, 1, -1, 1, 1])
    with pytest.raises(ValueError, match="l1_weights: entries must be finite"):
        R.ADMMmethod(X, y, l1_weights=[1, 1, float("nan"), 1, 1])
    with pytest.raises(ValueError, match="must hold a positive penalty"):
        R.ADMMmethod(X, y, l1_weights=np.zeros(5))
    with pytest.raises(ValueError, match="smoothADMMmethod has no per-coordinate penalties"):
        R.smoothADMMmethod(X, y, l1_reg=0.1, l1_weights=np.ones(5))
    with pytest.raises(ValueError, match="smoothADMMmethod has no per-coordinate penalties"):
        R.smoothADMMmethod(X, y, l1_reg=0.1, fit_intercept=True)
    with pytest.raises(ValueError, match="problem 1: l2_weights: has 3 entries"):
        R.ADMMgroup(X, y, [dict(l1_reg=0.1), dict(l2_weights=np.ones(3))])
    with pytest.raises(ValueError, match="fit_intercept must be the same"):
        R.ADMMgroup(X, y, [dict(l1_reg=0.1), dict(l1_reg=0.1, fit_intercept=True)])


def test_resolved_penalty_rules():
    from admm_for_rank_based_loss_amd import _solver, _lib
    assert _solver.resolve_penalty(3, l1_reg=0.1) is None                         # nothing new given: the scalar path
    p = _solver.resolve_penalty(3, l1_reg=0.1, fit_intercept=True)
    assert p["l1"].tolist() == [0.1, 0.1, 0.1, 0.0] and p["l2"].tolist() == [0.0] * 4
    assert p["wstep"] == _lib.WSTEP_L1 and p["reg"] == 0.1                          # starts where l1_reg=0.1 does
    p = _solver.resolve_penalty(3, l1_reg=0.1, l2_reg=0.3, fit_intercept=True)      # the reference's rule: l1_reg wins
    assert p["l2"].tolist() == [0.0] * 4 and p["wstep"] == _lib.WSTEP_L1
    p = _solver.resolve_penalty(3, l2_weights=[1.0, 0.0, 2.0])
    assert p["wstep"] == _lib.WSTEP_L2 and p["reg"] == 1.0 and p["l1"].tolist() == [0.0] * 3
    p = _solver.resolve_penalty(3, l1_weights=0.25, l2_weights=[1.0, 0.0, 2.0])
    assert p["wstep"] == _lib.WSTEP_L1 and p["reg"] == 0.25 and p["l1"].tolist() == [0.25] * 3
