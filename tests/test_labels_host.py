"""CPU-only checks of members with labels of their own on one data matrix (include/rbl.h: rbl_set_labels,
rbl_decide_multi; ADMMgroup problems with a ``y``; OneVsRest): the two symbols in header, library and binding with the
ABI unchanged, argument validation before any device call, no CPU fallback, and the sign-convention identities the
kernels implement, checked on the NumPy oracle to the last bit of w."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT


def _pkg():
    import admm_for_rank_based_loss_amd as rbl
    return rbl


def test_new_symbols_in_header_library_and_binding():
    rbl = _pkg()
    header = open(os.path.join(ROOT, "include", "rbl.h")).read()
    lib = rbl._lib.load()
    for name in ("rbl_set_labels", "rbl_decide_multi"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
        assert name in rbl._lib.SIGNATURES, name
    assert callable(rbl.Solver.set_labels) and callable(rbl.Solver.decide_multi)
    assert "OneVsRest" in rbl.__all__ and rbl.OneVsRest is not None
    # nothing that exists moved: version, structure sizes, the last constructor keyword, ADMMgroup's parameters
    assert lib.rbl_version() == 106
    assert "#define RBL_VERSION 106" in header
    assert lib.rbl_sizeof(0) == C.sizeof(rbl._lib.RblConfig) == 136
    assert lib.rbl_sizeof(1) == C.sizeof(rbl._lib.RblStats) == 112
    import inspect
    assert list(inspect.signature(rbl.ADMMmethod.__init__).parameters)[-1] == "share_data"
    assert list(inspect.signature(rbl.smoothADMMmethod.__init__).parameters)[-1] == "share_data"
    assert list(inspect.signature(rbl.ADMMgroup.__init__).parameters) == ["self", "X", "y", "problems", "storage", "device",
                                                                          "max_iter", "tol"]


def _fake_owner(rbl, n, d, storage="f32"):
    """what Optimizer.__init__ looks at in share_data before it creates a handle - no device behind it"""
    s = object.__new__(rbl.Solver)
    s._h = None
    s.n, s.d, s.n_total = n, d, n
    cfg = rbl._lib.RblConfig()
    cfg.storage = rbl._lib.STORAGE[storage]
    cfg.device = 0
    s.cfg = cfg
    return s


def test_argument_validation_before_any_device_call():
    rbl = _pkg()
    rng = np.random.default_rng(0)
    X = rng.standard_normal((12, 3))
    y = np.where(rng.standard_normal(12) > 0, 1.0, -1.0)
    base = dict(weight_function="superquantile", loss="binary_cross_entropy", l2_reg=0.1, args=[0.5])
    bad_value = y.copy()
    bad_value[5] = 0.5
    # ADMMgroup: a member's y of the wrong length / with a value outside +-1, naming the problem
    with pytest.raises(ValueError, match=r"problem 1: .*11 labels for 12 rows"):
        rbl.ADMMgroup(X, y, [dict(base), dict(base, y=y[:11])])
    with pytest.raises(ValueError, match=r"problem 2: .*labels must be \+1/-1"):
        rbl.ADMMgroup(X, y, [dict(base), dict(base, y=-y), dict(base, y=bad_value)])
    # share_data: the same checks in the constructor, before a handle is created
    owner = _fake_owner(rbl, 12, 3)
    with pytest.raises(ValueError, match="11 labels for 12 rows"):
        rbl.ADMMmethod(X, y[:11], share_data=owner, **base)
    with pytest.raises(ValueError, match=r"labels must be \+1/-1"):
        rbl.smoothADMMmethod(X, bad_value, share_data=owner, weight_function="erm", l1_reg=0.1)
    # OneVsRest: a single class, labels of the wrong length
    with pytest.raises(ValueError, match="at least 2 classes"):
        rbl.OneVsRest(X, np.zeros(12), l2_reg=0.1)
    with pytest.raises(ValueError, match="11 entries for 12 rows"):
        rbl.OneVsRest(X, np.arange(11) % 3, l2_reg=0.1)
    # start_store with a list of test labels: its length and every entry are checked before a test objective is built
    g = object.__new__(rbl.ADMMgroup)
    g.solvers, g.problems = [None] * 3, [dict(base)] * 3
    Xt = rng.standard_normal((7, 3))
    yt = np.where(rng.standard_normal(7) > 0, 1.0, -1.0)
    with pytest.raises(ValueError, match=r"problem 2: y_test lists 2 label arrays for 3 problems"):
        g.start_store(Xt, [yt, -yt])
    with pytest.raises(ValueError, match=r"problem 1: .*6 labels for 7 rows"):
        g.start_store(Xt, [yt, yt[:6], yt])
    with pytest.raises(ValueError, match=r"problem 2: .*labels must be \+1/-1"):
        g.start_store(Xt, [yt, -yt, 3.0 * yt])
    # Solver.set_labels / decide_multi check shapes before the library is called
    s = _fake_owner(rbl, 12, 3)
    with pytest.raises(ValueError, match="11 labels for 12 rows"):
        s.set_labels(y[:11])
    with pytest.raises(ValueError, match=r"labels must be \+1/-1"):
        s.set_labels(bad_value)
    with pytest.raises(ValueError, match=r"W must be \(k, 3\)"):
        s.decide_multi(np.zeros((2, 4)))
    with pytest.raises(ValueError, match=r"W must be \(k, 3\)"):
        s.decide_multi(np.zeros((65, 3)))


def test_relabelled_group_has_no_cpu_fallback():
    """a valid group whose members carry labels of their own: without a GPU the first handle fails loudly"""
    rbl = _pkg()
    rng = np.random.default_rng(1)
    X = rng.standard_normal((40, 4))
    ys = [np.where(rng.standard_normal(40) > 0, 1.0, -1.0) for _ in range(3)]
    probs = [dict(weight_function="superquantile", loss="binary_cross_entropy", l2_reg=0.1, args=[0.5], y=yk) for yk in ys]
    if rbl._lib.device_count() > 0:
        g = rbl.ADMMgroup(X, ys[0], probs, storage="f64", max_iter=2)     # with a GPU the same call simply works
        assert [np.array_equal(s._s.labels(), yk) for s, yk in zip(g.solvers, ys)] == [True] * 3
        g.close()
        return
    with pytest.raises(rbl._lib.RblError, match="no HIP device"):
        rbl.ADMMgroup(X, ys[0], probs, storage="f64", max_iter=2)
    with pytest.raises(rbl._lib.RblError, match="no HIP device"):
        rbl.OneVsRest(X, np.arange(40) % 3, l2_reg=0.1)


@pytest.mark.parametrize("pr", [
    dict(weight_function="superquantile", loss="binary_cross_entropy", l2_reg=0.01, args=[0.5]),
    dict(weight_function="extremile", loss="binary_cross_entropy", l1_reg=0.01, args=[2.0]),
    dict(weight_function="aorr", loss="hinge", l2_reg=1e-4, args=[0.2, 0.8]),
    dict(weight_function="erm", loss="hinge", l2_reg=0.01),
    dict(weight_function="ehrm", loss="binary_cross_entropy", l2_reg=0.01, B=-5),
], ids=lambda p: f"{p['weight_function']}_{p['loss']}")
def test_sign_convention_identities_on_the_oracle(pr):
    """Exact ADMM iterations on (X, y_k) against the same iterations carried out on the OWNER's D_0 = -y_0*X with the
    state kept as z~ = r z, lambda~ = r lambda (r = y_k*y_0): v_raw = D_0 w, m = r (v_raw - lambda~/rho), z~ = r z,
    q = D_0^T (z~ + lambda~/rho), lambda~ += rho (z~ - v_raw), primal = ||z~ - v_raw||, G = D_0^T D_0.  Negation is
    exact and every sum is the same chain of the same products, so w, z, lambda and rho agree to the last bit."""
    from oracle import admm, weights, wstep
    rng = np.random.default_rng(42)
    n, d, nit = 300, 7, 8
    X = rng.standard_normal((n, d))
    y0 = np.where(rng.standard_normal(n) > 0, 1.0, -1.0)
    yk = np.where(rng.standard_normal(n) > 0, 1.0, -1.0)
    r = yk * y0
    assert (r > 0).any() and (r < 0).any()
    ref = admm.admm_solve(X, yk, max_iter=nit, mode="exact", tol=0.0, **pr)

    loss, wf = pr["loss"], pr["weight_function"]
    sa, sb = weights.get_weights(wf, n, pr.get("args"))
    D0 = -y0.reshape(-1, 1) * X
    Dk = -yk.reshape(-1, 1) * X
    G = D0.T @ D0
    assert np.array_equal(G, Dk.T @ Dk)            # the Gram matrix does not depend on the labels
    reg = pr.get("l1_reg") or pr.get("l2_reg")
    lam_t = r * (0.1 * reg / n * np.ones(n))
    z_t = r * (0.1 * reg / n * np.ones(n))
    w = 0.001 * reg / d / n * np.ones(d)
    rho = admm.initial_rho(wf)
    L = 1.0001 * wstep.lambda_max(G)
    v_raw = D0 @ w
    for it in range(nit):
        m = r * (v_raw - lam_t / rho)
        z, _ = admm.z_step_exact(wf, loss, sa, sb, pr.get("B"), rho, m)
        z_t = r * z
        q = D0.T @ (z_t + lam_t / rho)
        if pr.get("l1_reg") is not None:
            w, _ = wstep.lasso_gram_exact(G, q, reg / (2.0 * rho), w, L, tol=1e-14)
        else:
            w = wstep.ridge_gram_exact(G, q, rho, reg)
        v_raw = D0 @ w
        lam_t = lam_t + rho * (z_t - v_raw)
        primal = float(np.linalg.norm(z_t - v_raw))
        assert rho == ref.rho[it], it
        assert primal == ref.primal[it], it
        rho = admm.next_rho(rho, primal, d)
    assert np.array_equal(w, ref.w)
    assert np.array_equal(r * z_t, ref.z)
    assert np.array_equal(r * lam_t, ref.lam)
