"""Row-weighted erm solves (sample_weight / class_weight; include/rbl.h: rbl_set_row_weights) on the GPU against the CPU
reference tests/weighted_ref.py run on the stored matrix: every route a weighted handle can take - the two-pass
iteration (narrow rows, RBL_NO_FUSE=1, storage="csr", group members), the single-sweep pass (wave-per-row and
workgroup-per-row kernels, rbl_stats.fused == 1) - for the three losses and the three w-steps; the logged objective
against math.fsum; c == 1 against the unweighted solve bit for bit; weights replaced between iterations; ADMMgroup with
0/1 fold masks; OneVsRest(class_weight="balanced"); the refusals of the C ABI; examples/run_cv_folds.py."""
import contextlib
import io
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import weighted_ref

pytestmark = pytest.mark.gpu

BCE, HINGE, SQ = "binary_cross_entropy", "hinge", "squared_hinge"


@pytest.fixture(scope="module")
def R():
    import admm_for_rank_based_loss_amd as rbl
    if rbl._lib.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run the HIP library (no fallback)")
    return rbl


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _weights(n, seed, zeros=0.2):
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.2, 3.0, size=n)
    c[rng.random(n) < zeros] = 0.0
    c[0] = 0.0
    return c


def _problem(n, d, seed, density=None):
    from oracle import problems
    X, y = problems.make_problem(n, d, seed=seed)
    if density is not None:
        X = X * (np.random.default_rng(seed + 1).random((n, d)) < density)
    return X, np.asarray(y, dtype=np.float64).reshape(-1)


def _stored_D(R, X, y, storage):
    """the matrix the device holds: -y * X rounded once to the storage type (csr keeps float64 entries)"""
    return R._lib.storage_round(-y.reshape(-1, 1) * X, "f64" if storage == "csr" else storage)


def _make(R, X, y, storage, kw, nit, smooth=False, no_fuse=False, **more):
    if no_fuse:
        os.environ["RBL_NO_FUSE"] = "1"          # read by rbl_create
    try:
        if storage == "csr":
            import scipy.sparse as sp
            X = sp.csr_matrix(X)
        cls = R.smoothADMMmethod if smooth else R.ADMMmethod
        return cls(X, y, max_iter=nit, tol=0.0, storage=storage, **kw, **more)
    finally:
        os.environ.pop("RBL_NO_FUSE", None)


def _tol(loss):
    return 1e-9 if loss == BCE else 1e-7        # test_iterates_match_oracle_exact's bar


def _check_against_ref(s, ref, D, c_of_iter, loss, kw, nit, first=0, want_fused=None, ctx=None):
    """iterations first .. first + nit - 1 of solver s against the reference trace, at test_iterates_match_oracle_exact's
    bar; the logged objective also against math.fsum on the device's own w (test_gpu_risk's bar)"""
    tol = _tol(loss)
    for i in range(first, first + nit):
        st = s._s.step(want_objective=True)
        assert abs(st.rho - ref.rho[i]) <= 1e-15 * ref.rho[i], (ctx, i)
        assert abs(st.primal - ref.primal[i]) <= tol * max(1.0, ref.primal[i]), (ctx, i, st.primal, ref.primal[i])
        assert abs(st.dual - ref.dual[i]) <= tol * max(1.0, ref.dual[i]), (ctx, i)
        assert abs(st.objective - ref.objective[i + 1]) <= tol * max(1.0, abs(ref.objective[i + 1])), (ctx, i)
        w = s._s.get_state(want_z=False, want_lam=False)["w"]
        exact = weighted_ref.objective(loss, c_of_iter(i), D @ w, w, kw.get("l2_reg"), kw.get("l1_reg"))
        assert abs(st.objective - exact) <= 1e-12 * max(1.0, abs(exact)), (ctx, i, st.objective, exact)
        if want_fused is not None and i >= 1:
            assert st.fused == want_fused, (ctx, i, st.fused)
    state = s._s.get_state()
    rw, rz, rl = ref.states[first + nit - 1]
    assert np.max(np.abs(state["w"] - rw)) <= tol * max(1.0, np.max(np.abs(rw))), ctx
    assert np.max(np.abs(state["z"] - rz)) <= 10 * tol * max(1.0, np.max(np.abs(rz))), ctx
    assert np.max(np.abs(state["lam"] - rl)) <= 10 * tol * max(1e-3, np.max(np.abs(rl))), ctx
    return state


# ------------------------------------------------------------------------------------------------ iterates
# (rows, cols, storage, loss, regulariser, smoothed w-step, density, fused from iteration 1 on)
SOLVES = [
    (300, 40, "f64", BCE, "l1_reg", False, None, 0),          # narrow rows: the two-pass iteration (k_erm_zc)
    (300, 40, "f64", HINGE, "l2_reg", False, None, 0),
    (300, 40, "f64", SQ, "l1_reg", True, None, 0),            # ... with the smoothed w-step
    (700, 200, "f32", BCE, "l1_reg", False, None, 1),         # wave-per-row kernel
    (700, 200, "f64", HINGE, "l2_reg", False, None, 1),
    (700, 200, "fp16", SQ, "l2_reg", False, None, 0),         # (fp16 rows of <= 256 elements are <= 32 packets: two-pass)
    (700, 264, "fp16", SQ, "l2_reg", False, None, 1),         # fp16 on the wave-per-row kernel: 33 packets per row
    (700, 200, "f64", HINGE, "l1_reg", True, None, 1),       # ... with the smoothed w-step
    (150, 2100, "f32", BCE, "l2_reg", False, None, 1),        # workgroup-per-row kernel
    (150, 2100, "f32", HINGE, "l1_reg", False, None, 1),
    (400, 60, "csr", BCE, "l1_reg", False, 0.2, 0),           # sparse storage: the two-pass iteration
    (400, 60, "csr", SQ, "l2_reg", False, 0.2, 0),
]


@pytest.mark.parametrize("n,d,storage,loss,reg,smooth,density,fused", SOLVES,
                         ids=[f"{s[0]}x{s[1]}-{s[2]}-{s[3]}-{s[4]}{'-smooth' if s[5] else ''}" for s in SOLVES])
def test_weighted_iterates_match_the_reference(R, n, d, storage, loss, reg, smooth, density, fused):
    if storage == "csr":
        pytest.importorskip("scipy.sparse")
    nit = 25
    X, y = _problem(n, d, 40 + d, density)
    c = _weights(n, 7 + n)
    kw = {reg: 0.01}
    D = _stored_D(R, X, y, storage)
    ref = weighted_ref.admm(X, y, c, loss, max_iter=nit, tol=0.0, smooth=smooth, D=D, **kw)
    s = _make(R, X, y, storage, dict(kw, loss=loss), nit, smooth=smooth, sample_weight=c)
    assert np.array_equal(s.sample_weight_, c) and np.array_equal(s._s.get_row_weights(), c)
    _check_against_ref(s, ref, D, lambda i: c, loss, kw, nit, want_fused=fused, ctx=(n, d, storage, loss, reg, smooth))
    # rbl_objective uses the weights too (train_losses[0] of start_store, the converged print)
    w = s._s.get_state(want_z=False, want_lam=False)["w"]
    exact = weighted_ref.objective(loss, c, D @ w, w, kw.get("l2_reg"), kw.get("l1_reg"))
    got = s.objective.get_arrogate_loss(w)
    assert abs(got - exact) <= 1e-12 * max(1.0, abs(exact)), (got, exact)
    s._s.close()


def test_start_store_logs_weighted_objectives(R):
    """train_losses carry the training weights; a test handle is unweighted unless it gets sample_weight_test"""
    n, nt, d, l2 = 300, 120, 40, 0.05
    X, y = _problem(n, d, 51)
    Xt, yt = _problem(nt, d, 52)
    c, ct = _weights(n, 3), _weights(nt, 4)
    D, Dt = -y.reshape(-1, 1) * X, -yt.reshape(-1, 1) * Xt
    for cw_test in (None, ct):
        s = R.ADMMmethod(X, y, "erm", BCE, l2_reg=l2, storage="f64", max_iter=6, tol=0.0, sample_weight=c)
        s.start_store(Xt, yt, "erm", BCE, l2_reg=l2, sample_weight_test=cw_test)
        _quiet(s.main_loop, verbose=False)
        w, _, train, test = s.final_res()
        w = np.asarray(w).reshape(-1)
        for got, exact in ((train[-1], weighted_ref.objective(BCE, c, D @ w, w, l2)),
                           (test[-1], weighted_ref.objective(BCE, cw_test, Dt @ w, w, l2))):
            assert abs(got - exact) <= 1e-12 * max(1.0, abs(exact)), (cw_test is None, got, exact)
        assert (s.test_objective.sample_weight_ is None) == (cw_test is None)
        s.test_objective._s.close()
        s._s.close()


# ------------------------------------------------------------------------------------------------ c == 1
@pytest.mark.parametrize("n,d,storage,fused", [(700, 200, "f32", 1), (300, 40, "f64", 0)], ids=["single_sweep", "two_pass"])
@pytest.mark.parametrize("loss", [BCE, HINGE, SQ])
def test_unit_weights_are_the_unweighted_solve_bit_for_bit(R, n, d, storage, fused, loss):
    X, y = _problem(n, d, 3)
    runs = []
    for sw in (None, np.ones(n)):
        s = _make(R, X, y, storage, dict(loss=loss, l1_reg=0.01), 20, sample_weight=sw)
        stats = []
        for i in range(20):
            st = s._s.step(want_objective=True)
            stats.append((st.primal, st.dual, st.rho, st.objective, st.fused, st.mispredicted, st.inner_iters))
            assert i == 0 or st.fused == fused
        runs.append((stats, s._s.get_state(), s.objective.get_arrogate_loss(s.w)))
        s._s.close()                            # one live handle at a time: the same form of the w-step on both sides
    (sa, a, fa), (sb, b, fb) = runs
    assert sa == sb
    for key in ("w", "z", "lam"):
        assert np.array_equal(a[key], b[key]), key
    assert a["rho"] == b["rho"] and fa == fb


# ------------------------------------------------------------------------------------------------ RBL_NO_FUSE
@pytest.mark.parametrize("loss", [BCE, HINGE, SQ])
def test_two_pass_route_equals_the_single_sweep_route(R, loss):
    """RBL_NO_FUSE=1 (k_erm_zc with sigma per row, the weighted loss sum behind k_dual) against the single-sweep weighted
    solve, at the bar test_single_sweep_paths holds its routes to"""
    n, d, nit = 700, 200, 30
    X, y = _problem(n, d, 9)
    c = _weights(n, 5)
    out = {}
    for name, nf in (("fused", False), ("unfused", True)):
        s = _make(R, X, y, "f64", dict(loss=loss, l1_reg=0.01), nit, no_fuse=nf, sample_weight=c)
        st = [s._s.step(want_objective=True) for _ in range(nit)]
        assert all(x.fused == (0 if nf else 1) for x in st[1:]), name
        out[name] = (s._s.get_state(), [x.objective for x in st])
        s._s.close()
    a, b = out["fused"][0], out["unfused"][0]
    assert np.max(np.abs(a["w"] - b["w"])) <= 1e-12
    assert np.max(np.abs(a["lam"] - b["lam"])) <= 1e-12 * max(1.0, np.max(np.abs(a["lam"])))
    assert np.allclose(out["fused"][1], out["unfused"][1], rtol=1e-12, atol=0.0)


# ------------------------------------------------------------------------------------------------ new weights mid-run
@pytest.mark.parametrize("n,d,storage", [(700, 200, "f64"), (300, 40, "f64")], ids=["single_sweep", "two_pass"])
def test_set_sample_weight_between_iterations(R, n, d, storage):
    """weights replaced after 5 iterations: the next 10 equal the reference that switches c at the same iteration (what
    the pass computed ahead with the old weights is dropped); None afterwards returns to the unweighted iterates"""
    X, y = _problem(n, d, 13)
    c1, c2 = _weights(n, 1), _weights(n, 2, zeros=0.4)
    kw = dict(l1_reg=0.01)
    D = _stored_D(R, X, y, storage)
    ref = weighted_ref.admm(X, y, {0: c1, 5: c2, 15: None}, BCE, max_iter=20, tol=0.0, D=D, **kw)
    cs = lambda i: c1 if i < 5 else (c2 if i < 15 else None)
    s = _make(R, X, y, storage, dict(kw, loss=BCE), 20, sample_weight=c1)
    _check_against_ref(s, ref, D, cs, BCE, kw, 5, first=0, ctx="c1")
    s.set_sample_weight(c2)
    assert np.array_equal(s.sample_weight_, c2) and np.array_equal(s._s.get_row_weights(), c2)
    _check_against_ref(s, ref, D, cs, BCE, kw, 10, first=5, ctx="c2")
    s.set_sample_weight(None)
    assert s.sample_weight_ is None and s._s.get_row_weights() is None
    _check_against_ref(s, ref, D, cs, BCE, kw, 5, first=15, ctx="none")
    s._s.close()


# ------------------------------------------------------------------------------------------------ ADMMgroup: folds
def test_group_members_with_fold_masks(R):
    """500 x 200 f32: three erm members with disjoint 0/1 fold masks and one unweighted member in one ADMMgroup; each
    against its standalone two-pass solver at the bar tests/test_gpu_group.py holds erm members to (1e-11 relative on w
    and lambda: the same maths, another order of the fp64 sums); the passes are shared"""
    n, d, nit = 500, 200, 12
    X, y = _problem(n, d, 21)
    fold = np.random.default_rng(4).permutation(n) % 3
    masks = [(fold != k).astype(np.float64) for k in range(3)] + [None]
    probs = [dict(weight_function="erm", loss=BCE, l1_reg=0.01, sample_weight=m) for m in masks]
    grp = R.ADMMgroup(X, y, probs, storage="f32", max_iter=nit, tol=0.0)
    for _ in range(nit):
        grp._group.step(want_objective=True)
    cnt = grp.counters()
    assert cnt["shared_v"] > 0 and cnt["shared_q"] > 0, cnt
    states = [s._s.get_state() for s in grp.solvers]
    for k, m in enumerate(masks):
        got = grp.solvers[k]._s.get_row_weights()
        assert (got is None) if m is None else np.array_equal(got, m)
        s = _make(R, X, y, "f32", dict(loss=BCE, l1_reg=0.01), nit, no_fuse=True, sample_weight=m)
        for _ in range(nit):
            assert s._s.step(False).fused == 0
        alone = s._s.get_state()
        dl = np.max(np.abs(states[k]["lam"] - alone["lam"])) / max(1e-3, np.max(np.abs(alone["lam"])))
        dw = np.max(np.abs(states[k]["w"] - alone["w"])) / max(1.0, np.max(np.abs(alone["w"])))
        print(f"fold member {k}: group vs standalone rel lam {dl:.2e} w {dw:.2e}")
        assert dl <= 1e-11 and dw <= 1e-11, (k, dl, dw)
        s._s.close()
    grp.close()


# ------------------------------------------------------------------------------------------------ OneVsRest
def test_one_vs_rest_balanced(R):
    sizes = (10, 30, 60, 100)
    n, d, nit = sum(sizes), 40, 10
    X, _ = _problem(n, d, 33)
    labels = np.repeat(np.arange(4), sizes)
    X = X + 0.5 * np.eye(4)[labels] @ np.random.default_rng(2).standard_normal((4, d))
    ovr = R.OneVsRest(X, labels, l2_reg=0.05, storage="f64", max_iter=nit, tol=0.0, class_weight="balanced")
    W = _quiet(ovr.main_loop, verbose=False)
    assert W.shape == (d, 4)
    for k, nk in enumerate(sizes):
        yk = np.where(labels == k, 1.0, -1.0)
        want = np.where(yk > 0, n / (2.0 * nk), n / (2.0 * (n - nk)))
        assert np.array_equal(ovr.group.solvers[k]._s.get_row_weights(), want), k
        assert np.array_equal(ovr.group.solvers[k].sample_weight_, want), k
        s = R.ADMMmethod(X, yk, l2_reg=0.05, storage="f64", max_iter=nit, tol=0.0, sample_weight=want)
        for _ in range(nit):
            s._s.step(False)
        w = s._s.get_state(want_z=False, want_lam=False)["w"]
        dw = np.max(np.abs(W[:, k] - w)) / max(1.0, np.max(np.abs(w)))
        assert dw <= 1e-11, (k, dw)
        s._s.close()
    pred = ovr.predict(X)                       # unchanged in form: a class label per row
    assert pred.shape == (n,) and set(np.unique(pred)) <= set(ovr.classes_.tolist())
    ovr.close()


# ------------------------------------------------------------------------------------------------ refusals of the C ABI
def test_c_abi_refusals(R):
    S, L = R._solver.Solver, R._lib
    s = S(60, 8, "superquantile", BCE, reg=0.01, args=[0.5])
    with pytest.raises(ValueError, match="PAV z-step does not apply"):
        s.set_row_weights(np.ones(60))
    s.close()
    s = S(30, 8, "erm", BCE, reg=0.01, n_total=60)
    with pytest.raises(ValueError, match="row-sharded"):
        s.set_row_weights(np.ones(30))
    s.close()
    s = S(30, 8, "erm", BCE, reg=0.01)
    for bad, word in ((-0.5, "c[3]"), (np.nan, "c[3]"), (np.inf, "c[3]")):
        c = np.ones(30)
        c[3] = bad
        c[7] = bad
        with pytest.raises(ValueError) as e:
            L.check(L.load().rbl_set_row_weights(s._h, L.ptr(c)))          # past the Python check: the library's own
        assert word in str(e.value), str(e.value)
    with pytest.raises(ValueError, match="zero"):
        L.check(L.load().rbl_set_row_weights(s._h, L.ptr(np.zeros(30))))
    assert s.get_row_weights() is None          # a refused call leaves the handle as it was
    s.set_row_weights(np.arange(30.0))
    assert np.array_equal(s.get_row_weights(), np.arange(30.0))
    s.set_row_weights(None)
    assert s.get_row_weights() is None
    s.close()


# ------------------------------------------------------------------------------------------------ the example
def test_run_cv_folds_example():
    env = dict(os.environ, RBL_EXAMPLE_FAST="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_cv_folds.py"), "--rows", "600", "--cols", "150"],
                       capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [ln.split(",") for ln in r.stdout.splitlines() if ln.count(",") == 4 and not ln.startswith("l1_reg")]
    assert len(rows) == 15, r.stdout
    assert all(math.isfinite(float(x[3])) and 0.5 < float(x[4]) <= 1.0 for x in rows), rows
    chosen = [ln for ln in r.stdout.splitlines() if ln.startswith("chosen,")]
    assert len(chosen) == 1 and float(chosen[0].split(",")[1]) in (0.1, 0.01, 0.001)
