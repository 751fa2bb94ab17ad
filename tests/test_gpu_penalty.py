"""Per-coordinate penalties on the GPU (include/rbl.h: rbl_set_penalty): R(w) = 1/2 sum_j (l1_j |w_j| + l2_j w_j^2) -
elastic net, penalty factors, free coordinates and the intercept built on them.  The w-step kernel entry against the
NumPy reference (tests/penalty_ref.py), whole solves against the same class with both sub-problem hooks overridden
(the construction of test_gpu_solver.py::test_overridden_subproblem_hooks, its bars), uniform vectors against the
scalar path, the intercept, groups, two ranks and the error codes."""
import contextlib
import io
import sys

import numpy as np
import pytest

from penalty_ref import enet_gram_exact, enet_kkt_residual, enet_objective

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    import admm_for_rank_based_loss_amd as rbl
    if rbl._lib.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run the HIP library (no fallback)")
    return rbl


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


# ------------------------------------------------------------------------------------ 1. the kernel entry
def _gram(d, seed):
    rng = np.random.default_rng(seed)
    D = rng.standard_normal((400, d))
    return rng, D.T @ D, D.T @ rng.standard_normal(400)


@pytest.mark.parametrize("d", [8, 60, 300])
def test_kernel_vs_reference(R, d):
    L = R._lib
    rng, G, q = _gram(d, 1000 + d)
    qm = np.max(np.abs(q))
    kbar = 1e-9 * max(1.0, qm)                              # test_gpu_widths.py:137
    close = lambda w, ref: np.max(np.abs(w - ref)) <= 1e-10 * max(1.0, np.max(np.abs(ref)))   # test_gpu_kernels.py:275
    rho = 0.5
    # uniform a: the scalar lasso kernel
    a = 2 * rho * 0.5 * qm
    w, _, form = L.k_wstep_pen(G, q, rho, l1=a)
    w_s, _ = L.k_wstep(1, G, q, rho, a)
    assert form == 2 and close(w, w_s)
    # a = 0, uniform b: the scalar ridge
    w, _, form = L.k_wstep_pen(G, q, rho, l2=0.3)
    w_s, _ = L.k_wstep(2, G, q, rho, 0.3)
    assert form in (0, 1) and close(w, w_s)
    # mixed a, b (all b > 0: unique) with one free coordinate
    l1 = 2 * rho * 0.4 * qm * rng.uniform(0.5, 2.0, d)
    l2 = rho * rng.uniform(0.1, 2.0, d)
    l1[2] = 0.0
    ref = enet_gram_exact(G, q, rho, l1, l2)
    w, _, form = L.k_wstep_pen(G, q, rho, l1, l2)
    assert form == 2 and enet_kkt_residual(G, q, rho, l1, l2, w) <= kbar and close(w, ref)
    assert w[2] != 0.0 and 0 < np.count_nonzero(w) < d
    # a free coordinate warm-started at +1 whose optimum is negative: the zero crossing is no break point
    q2 = q.copy()
    q2[2] = -3.0 * qm
    ref = enet_gram_exact(G, q2, rho, l1, l2)
    assert ref[2] < 0
    w0 = np.zeros(d)
    w0[2] = 1.0
    w, _, form = L.k_wstep_pen(G, q2, rho, l1, l2, w0=w0)
    assert form == 2 and w[2] < 0 and close(w, ref)
    assert enet_kkt_residual(G, q2, rho, l1, l2, w) <= 1e-9 * max(1.0, np.max(np.abs(q2)))
    # kappa so large that every penalised coordinate is exactly 0.0 while the free one is not
    big = np.full(d, 2 * rho * 50.0 * qm)
    big[2] = 0.0
    w0 = np.zeros(d)
    w0[:6] = 0.01 * rng.standard_normal(6)          # (a warm start inside the kernel's capacity: they all have to leave)
    w, _, form = L.k_wstep_pen(G, q, rho, big, None, w0=w0)
    assert form == 2 and np.all(np.delete(w, 2) == 0.0) and w[2] != 0.0
    assert abs(w[2] - q[2] / G[2, 2]) <= 1e-10 * max(1.0, abs(q[2] / G[2, 2]))
    assert enet_kkt_residual(G, q, rho, big, None, w) <= kbar


def test_kernel_support_beyond_the_active_set_capacity(R):
    """d = 300 with a small kappa: the support exceeds the kernel's 96 coordinates and FISTA takes over (form 0);
    the objective is compared one-sidedly at 1e-10 relative, as test_gpu_kernels.py:340 does"""
    d = 300
    rng, G, q = _gram(d, 77)
    rho = 0.5
    l1 = 2 * rho * 0.01 * np.max(np.abs(q)) * rng.uniform(0.5, 2.0, d)
    l2 = rho * rng.uniform(0.1, 2.0, d)
    l1[2] = 0.0
    ref = enet_gram_exact(G, q, rho, l1, l2)
    assert np.count_nonzero(ref) > 96
    w, _, form = R._lib.k_wstep_pen(G, q, rho, l1, l2)
    assert form == 0
    f, fr = enet_objective(G, q, rho, l1, l2, w), enet_objective(G, q, rho, l1, l2, ref)
    assert f <= fr + 1e-10 * abs(fr) + 1e-12


# ------------------------------------------------------------------------------------ 2. whole solves
def _hooked(R, X, y, kw, l1, l2):
    """the same class with both sub-problem hooks answered in NumPy: the exact z-step and tests/penalty_ref.py"""
    from oracle import admm, weights
    n = X.shape[0]
    wf, loss = kw["weight_function"], kw["loss"]
    sa, sb = weights.get_weights(wf, n, kw.get("args"))
    D = -y.reshape(-1, 1) * X
    G = D.T @ D

    def z_hook(self):
        m = (D @ self.w - self.lagrangian / self.rho).reshape(-1)
        if loss == "squared_hinge":             # the oracle has no squared hinge: the project's restatement of it
            import sqhinge_ref
            return sqhinge_ref.z_step(wf, sa, self.rho, m).reshape(-1, 1)
        return admm.z_step_exact(wf, loss, sa, sb, None, self.rho, m)[0].reshape(-1, 1)

    def w_hook(self):
        rho = self.rho
        q = D.T @ (self.z + self.lagrangian / rho).reshape(-1)
        return enet_gram_exact(G, q, rho, l1, l2, self.w.reshape(-1)).reshape(-1, 1)

    class Hooked(R.ADMMmethod):
        z_subproblem = z_hook
        w_subproblem = w_hook

    return Hooked


def _run(R, cls, X, y, kw, nit, **extra):
    s = cls(X, y, max_iter=nit, tol=0.0, storage="f64", **kw, **extra)
    stats = []
    for i in range(nit):
        _quiet(R.Optimizer.main_loop, s, i, 0.0, True)        # verbose: the logged objective is computed
        stats.append(s._last)
    return s, stats


def _agree(a, sa, b, sb, tol):
    for x, yv, floor in ((a.w, b.w, 1.0), (a.z, b.z, 1.0), (a.lagrangian, b.lagrangian, 1e-3)):
        assert np.max(np.abs(x - yv)) <= tol * max(floor, np.max(np.abs(yv)))
    for s1, s2 in zip(sa, sb):
        assert abs(s1.primal - s2.primal) <= tol * max(1.0, s2.primal)
        assert abs(s1.dual - s2.dual) <= tol * max(1.0, s2.dual)
        assert abs(s1.rho - s2.rho) <= 1e-15 * s2.rho
        assert abs(s1.objective - s2.objective) <= tol * max(1.0, abs(s2.objective))


def _cases(d):
    rng = np.random.default_rng(d)
    l2free = np.full(d, 0.02)
    l2free[3] = 0.0
    return {
        "erm_bce_enet": (dict(weight_function="erm", loss="binary_cross_entropy"),
                         dict(l1_weights=0.01, l2_weights=0.02), (2,)),
        "superq_sqhinge_l2_free": (dict(weight_function="superquantile", loss="squared_hinge", args=[0.5]),
                                   dict(l2_weights=l2free), (0, 1)),
        "aorr_hinge_enet_factors": (dict(weight_function="aorr", loss="hinge", args=[0.2, 0.8]),
                                    dict(l1_weights=0.01 * rng.uniform(0.5, 2.0, d), l2_weights=0.02 * rng.uniform(0.5, 2.0, d)),
                                    (2,)),
    }


@pytest.mark.parametrize("d", [60, 200])
@pytest.mark.parametrize("name", ["erm_bce_enet", "superq_sqhinge_l2_free", "aorr_hinge_enet_factors"])
def test_whole_solves_match_the_hooked_reference(R, name, d):
    """1200 x 60 runs the two-sweep iteration, 1200 x 200 the single-sweep pass with the w-step enqueued ahead (erm)"""
    from oracle import problems
    from admm_for_rank_based_loss_amd import _solver
    X, y = problems.make_problem(1200, d, seed=91)
    kw, pen, forms = _cases(d)[name]
    nit = 12
    p = _solver.resolve_penalty(d, **pen)
    s, st = _run(R, R.ADMMmethod, X, y, kw, nit, **pen)
    h, sth = _run(R, _hooked(R, X, y, kw, p["l1"], p["l2"]), X, y, kw, nit, **pen)
    _agree(s, st, h, sth, 1e-7 if kw["loss"] == "hinge" else 1e-9)
    # iteration 0 starts from the reference's dense w (algorithms.py:42): at d = 200 its support is beyond the active-set
    # kernel's 96 coordinates and the (unchanged) hand-over to FISTA reports form 0, as it does on the scalar path
    first = forms + (0,) if d > 96 else forms
    assert st[0].wstep_form in first and all(x.wstep_form in forms for x in st[1:]), [x.wstep_form for x in st]
    assert all(x.wstep_form == -1 for x in sth)
    if kw["weight_function"] == "erm" and d == 200:
        assert all(x.fused == 1 for x in st[1:]), [x.fused for x in st]
    if forms == (0, 1) and d == 60:
        # a second live handle: the batched CG (form 0) instead of the persistent launch
        s2, st2 = _run(R, R.ADMMmethod, X, y, kw, nit, **pen)
        assert all(x.wstep_form == 0 for x in st2), [x.wstep_form for x in st2]
        _agree(s2, st2, h, sth, 1e-9)
        got = s._s.get_penalty()
        assert np.array_equal(got[0], p["l1"]) and np.array_equal(got[1], p["l2"])


# ------------------------------------------------------------------------------------ 3. uniform vectors = scalars
@pytest.mark.parametrize("which,d", [("l1", 60), ("l1", 200), ("l2", 60)])
def test_uniform_weights_equal_the_scalar_path(R, which, d):
    from oracle import problems
    X, y = problems.make_problem(1200, d, seed=5)
    kw = dict(weight_function="erm", loss="binary_cross_entropy")
    a, sa = _run(R, R.ADMMmethod, X, y, kw, 12, **{which + "_weights": 0.01})
    b, sb = _run(R, R.ADMMmethod, X, y, kw, 12, **{which + "_reg": 0.01})
    assert a._s.get_penalty() is not None and b._s.get_penalty() is None
    _agree(a, sa, b, sb, 1e-9)
    w = b.w
    assert abs(a.objective.get_arrogate_loss(w) - b.objective.get_arrogate_loss(w)) <= 1e-9 * abs(b.objective.get_arrogate_loss(w))


# ------------------------------------------------------------------------------------ 4. the intercept
def _imbalanced(n, d, seed, classes=2):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    X = (X - X.mean(axis=0)) / X.std(axis=0)
    score = X[:, :3] @ np.array([1.0, -0.5, 0.25]) + 0.3 * rng.standard_normal(n)
    y = np.where(score > np.quantile(score, 0.85), 1.0, -1.0)       # 85 % / 15 %
    return rng, X, y


def test_intercept(R):
    from admm_for_rank_based_loss_amd import _solver
    rng, X, y = _imbalanced(1200, 60, 3)
    kw = dict(weight_function="erm", loss="binary_cross_entropy")
    nit = 12
    s, st = _run(R, R.ADMMmethod, X, y, kw, nit, l1_reg=0.01, fit_intercept=True)
    Xa = np.hstack([X, np.ones((1200, 1))])
    p = _solver.resolve_penalty(60, l1_reg=0.01, fit_intercept=True)
    # the hooked reference: its NumPy sub-problems are those of the augmented matrix [X | 1] (same starting values)
    h, sth = _run(R, _hooked(R, Xa, y, kw, p["l1"], p["l2"]), X, y, kw, nit, l1_reg=0.01, fit_intercept=True)
    _agree(s, st, h, sth, 1e-9)
    w = s.w.reshape(-1)
    assert w.shape == (61,) and s.coef_.shape == (60,) and s.intercept_ != 0.0 and s.intercept_ == w[-1]
    assert np.array_equal(s.coef_, w[:-1])
    # accuracy on the augmented test matrix (src/util/calculate_acc.py: sigmoid(x . w) > 1/2 against y = +1)
    Xt = np.hstack([X[:300], np.ones((300, 1))])
    t = R.Solver(300, 61, "erm", "binary_cross_entropy", storage="f64", objective_only=True)
    t.set_data(Xt, y[:300])
    assert t.accuracy(w) == pytest.approx(float(np.mean(np.where(Xt @ w > 0, 1.0, -1.0) == y[:300])), abs=1e-12)
    t.close()
    # start_store appends the column to the test matrix as well
    s2 = R.ADMMmethod(X, y, max_iter=2, tol=0.0, storage="f64", l1_reg=0.01, fit_intercept=True, **kw)
    s2.start_store(X[:300], y[:300], l1_reg=0.01, **kw)
    assert np.isfinite(s2.test_losses[0])


def test_one_vs_rest_with_intercept(R):
    rng = np.random.default_rng(8)
    X = rng.standard_normal((1200, 20))
    lab = np.argmax(X[:, :3] + np.array([1.5, 0.0, -1.0]) + 0.3 * rng.standard_normal((1200, 3)), axis=1)
    ovr = R.OneVsRest(X, lab, l2_reg=0.01, storage="f64", max_iter=12, tol=0.0, fit_intercept=True)
    W = _quiet(ovr.main_loop, verbose=False)
    assert W.shape == (21, 3) and np.all(W[-1] != 0.0)
    Xt = np.hstack([X, np.ones((1200, 1))])
    scores = Xt @ W
    top = np.sort(scores, axis=1)
    keep = (top[:, -1] - top[:, -2]) >= 1e-13 * np.max(np.abs(Xt) @ np.abs(W) + 1, axis=1)   # test_gpu_labels.py's bound
    assert np.mean(~keep) <= 0.01
    pred = ovr.predict(X)
    assert np.array_equal(pred[keep], ovr.classes_[np.argmax(scores, axis=1)][keep])
    ovr.close()


# ------------------------------------------------------------------------------------ 5. group
def test_group_members_with_penalties_equal_standalone(R):
    """a scalar l1_reg, an elastic net and an l2 vector with a free coordinate on one (X, y): each member equals its
    standalone solver (erm outside the single-sweep pass, as inside a group) at test_gpu_group.py's 1e-11 relative, and
    the passes are shared as for scalar members"""
    import os
    from oracle import problems
    n, d, nit = 3000, 160, 10
    X, y = problems.make_problem(n, d, seed=260)
    l2free = np.full(d, 0.02)
    l2free[7] = 0.0
    members = [dict(weight_function="superquantile", loss="binary_cross_entropy", args=[0.5], l1_reg=0.01),
               dict(weight_function="superquantile", loss="binary_cross_entropy", args=[0.5], l1_weights=0.01, l2_weights=0.02),
               dict(weight_function="aorr", loss="hinge", args=[0.2, 0.8], l2_weights=l2free)]
    g = R.ADMMgroup(X, y, members, storage="f64", max_iter=nit, tol=0.0)
    for _ in range(nit):
        stats = g._group.step(want_objective=False)
    cnt = g.counters()
    K, kpp = len(members), cnt["k_per_pass"]
    assert kpp >= 2 and cnt["shared_v"] == cnt["shared_q"] == nit * -(-K // kpp), cnt
    assert [st.wstep_form for st in stats] == [2, 2, 0]
    states = [s._s.get_state() for s in g.solvers]
    for k, pr in enumerate(members):          # (the group's handles stay alive: the same form of the CG on both sides)
        s = R.ADMMmethod(X, y, max_iter=nit, tol=0.0, storage="f64", **pr)
        for _ in range(nit):
            s._s.step(False)
        alone = s._s.get_state()
        dl = np.max(np.abs(states[k]["lam"] - alone["lam"])) / max(1e-3, np.max(np.abs(alone["lam"])))
        dw = np.max(np.abs(states[k]["w"] - alone["w"])) / max(1.0, np.max(np.abs(alone["w"])))
        assert dl <= 1e-11 and dw <= 1e-11, (k, dl, dw)
        s._s.close()
    g.close()


# ------------------------------------------------------------------------------------ 6. two ranks
def test_two_ranks_as_threads_match_single_handle(R):
    """erm elastic net, rows sharded over two ranks run as threads on one GPU (the rig of tests/test_gpu_dist.py): the
    replicated w-step gets the same vectors on both ranks; w 1e-9, z 1e-8, the history 1e-8 - that file's bars"""
    import threading
    import torch
    from test_gpu_dist import _Hub, _make_thread_driver
    from admm_for_rank_based_loss_amd.dist import ShardedADMM, GpuEngine, shard_rows
    n, d, iters, world = 20000, 48, 8, 2
    l1 = np.full(d, 0.01)
    l2 = np.linspace(0.0, 0.04, d)
    mk = lambda cnt, lo: R.Solver(cnt, d, "erm", "binary_cross_entropy", reg=0.01, wstep=1, n_total=n, row_offset=lo,
                                  tol=0.0, storage="f64")

    def drive(drv, s):
        drv.setup_synthetic(seed=12)
        drv.setup_gram()
        hist = []
        for _ in range(iters):
            st = drv.step(True)
            hist.append((st.primal, st.dual, st.rho, st.objective))
        state = s.get_state()
        return dict(w=state["w"], z=state["z"], hist=np.array(hist))

    torch.cuda.set_device(0)
    s1 = mk(n, 0)
    one = drive(ShardedADMM(GpuEngine(s1, 0), world=1, rank=0, l1_weights=l1, l2_weights=l2), s1)
    s1.close()
    hub, out, errs = _Hub(world), [None] * world, []

    def rank_main(rank):
        try:
            torch.cuda.set_device(0)
            lo, cnt, _ = shard_rows(n, world, rank)
            s = mk(cnt, lo)
            drv = _make_thread_driver(ShardedADMM, hub)(GpuEngine(s, 0), world=world, rank=rank, l1_weights=l1, l2_weights=l2)
            out[rank] = drive(drv, s)
        except BaseException as e:       # a dead thread must not leave the other in a barrier forever
            errs.append((rank, repr(e)))
            hub.bar.abort()

    ts = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(120)
    assert not errs, errs
    assert np.array_equal(out[0]["w"], out[1]["w"]) and np.array_equal(out[0]["hist"], out[1]["hist"])
    z2 = np.concatenate([r["z"] for r in out])
    assert np.max(np.abs(out[0]["w"] - one["w"])) <= 1e-9 * max(1.0, np.max(np.abs(one["w"])))
    assert np.max(np.abs(z2 - one["z"])) <= 1e-8 * max(1.0, np.max(np.abs(one["z"])))
    assert np.allclose(out[0]["hist"], one["hist"], rtol=1e-8, atol=1e-12)
    # the objective carries the elastic net's R, not the scalar's
    w = one["w"]
    assert one["hist"][-1, 3] > 0.5 * np.sum(l1 * np.abs(w) + l2 * w * w)


# ------------------------------------------------------------------------------------ 7. errors
def test_error_codes(R):
    import ctypes as C
    from oracle import problems
    L = R._lib
    lib = L.load()
    X, y = problems.make_problem(200, 12, seed=1)
    s = R.ADMMmethod(X, y, l1_reg=0.01, storage="f64")._s
    ones = np.ones(12)
    neg = ones.copy()
    neg[4] = -1.0
    nan = ones.copy()
    nan[0] = np.nan
    for a, b in ((neg, None), (None, neg), (nan, None), (None, None)):
        assert lib.rbl_set_penalty(s._h, L.ptr(a), L.ptr(b)) == L.RBL_ERR_INVALID
        assert "set_penalty" in L.last_error()
    assert s.get_penalty() is None
    assert lib.rbl_set_penalty(s._h, L.ptr(ones), None) == L.RBL_OK
    assert np.array_equal(s.get_penalty()[0], ones) and np.array_equal(s.get_penalty()[1], np.zeros(12))
    s.step()
    assert lib.rbl_set_penalty(s._h, L.ptr(ones), None) == L.RBL_ERR_STATE
    assert "iterated" in L.last_error()
    sm = R.smoothADMMmethod(X, y, l1_reg=0.01, storage="f64")._s
    assert lib.rbl_set_penalty(sm._h, L.ptr(ones), None) == L.RBL_ERR_INVALID
    assert "smoothed-l1" in L.last_error()
    with pytest.raises(ValueError):
        L.k_wstep_pen(np.eye(3), np.ones(3), 1.0, l1=[1.0, -1.0, 1.0])
    # objective_only handles take the vectors: rbl_objective(include_reg) carries the same R
    o = R.Solver(200, 12, "erm", "binary_cross_entropy", storage="f64", objective_only=True)
    o.set_data(X, y)
    l2 = np.linspace(0.0, 1.0, 12)
    o.set_penalty(ones, l2)
    w = np.cos(np.arange(12.0))
    assert o.objective(w) == pytest.approx(o.risk(w) + 0.5 * np.sum(ones * np.abs(w) + l2 * w * w), rel=1e-13)
