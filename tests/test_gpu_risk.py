"""The numbers a user reads - the logged objective sum_k sigma_k loss(v_(k)), the accuracy, the six fairness statistics -
on PRESCRIBED scores against exact references (tests/risk_fixtures.py: the patterns, laid out around each family's band
edges, and risk_exact / accuracy_ref / fair_ref; test_risk_host.py pins what the fixtures claim).

    path A  mean          erm                                              k_loss_sum                   risk_path 1
    path B  sort + dot    smooth families; banded families under RBL_NO_ZBAND=1 and on an objective-only handle
                                                                           k_loss_keys, radix sort, k_sorted_loss_dot   2
    path C  select        banded families, RBL_ZBAND_MIN_N=16, after one step    k_zb_risk, k_zb_risk_finish            3
    path D  relabelled    a borrower with labels of its own (rs_flip, RS = true) on A, B and C
    path E  row-sharded   2 and 4 ranks as threads: rbl_zd_sort_losses, rbl_zd_risk, ShardedADMM._risk_distributed

v goes in through Solver.risk_from_v (a float64 device tensor) and, for rbl_objective / rbl_accuracy /
rbl_fair_statistics, through a one-column fp64 problem X[:, 0] = -y * v, w = [1].  Bar: |got - exact| <= 1e-12 max(1,
|exact|), the project's bar for the objective; every value finite.  Every case prints its error, pattern and
risk_path() before it is asserted (pytest -s)."""
import math

import numpy as np
import pytest

import risk_fixtures as F
import zstep_inject as Z

pytestmark = pytest.mark.gpu

ENV = {"sorted": {"RBL_NO_ZBAND": "1", "RBL_NO_SORT32": "0"},
       "select": {"RBL_NO_ZBAND": "0", "RBL_NO_SORT32": "0", "RBL_ZBAND_MIN_N": "16"}}
HANDLES = {}                      # (kind, family, loss, n) -> Solver
REF = {}                          # (family, loss, n, pattern, case, relabelled) -> exact risk
OBJECTIVE_PATTERNS = ["gaussian", "all_equal", "signed_zeros", "hinge_plateau", "extremes"]
RELABELLED_PATTERNS = ["gaussian", "all_equal", "span_one_edge", "signed_zeros"]
SHARDED_PATTERNS = ["gaussian", "all_equal", "two_values", "dup33"]


@pytest.fixture(scope="module")
def R():
    import admm_for_rank_based_loss_amd as rbl
    if rbl._lib.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run the HIP library (no fallback)")
    yield rbl
    for s in HANDLES.values():
        s.close()
    HANDLES.clear()


def _setenv(monkeypatch, kind):
    for k, v in ENV[kind].items():
        monkeypatch.setenv(k, v)


def _device(v):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float64)).to(torch.device("cuda", 0))
    torch.cuda.synchronize()                  # the handle runs on a stream of its own
    return t


def _one_column(R, fam, loss, v, y=None, share=None, labels=None):
    """an objective-only fp64 handle on X[:, 0] = -y * v, so that D w = v for w = [1] (a borrower: on the owner's data,
    with labels of its own)"""
    n = v.size
    wf, args, B = F.family(fam, n)
    s = R.Solver(n, 1, wf, loss, reg=0.0, B=B, args=args, storage="f64", objective_only=True, share=share)
    if share is None:
        y = np.ones(n) if y is None else y
        s.set_data((-y * v).reshape(n, 1), y)
    elif labels is not None:
        s.set_labels(labels)
    return s


def _stepped(R, monkeypatch, kind, fam, loss, n, share=None, labels=None):
    """a handle (data of zstep_inject.make_problem, or a relabelled borrower of `share`) after exactly ONE step() from
    iteration 1 on a gaussian m - the step that reads the environment and classifies sigma (zb_setup).  -> (solver,
    stats.zband of that step)"""
    _setenv(monkeypatch, kind)
    wf, args, B = F.family(fam, n)
    if share is None:
        X, y = Z.make_problem(n)
        s = R.Solver(n, 3, wf, loss, reg=0.01, wstep=2, args=args, B=B, tol=0.0, storage="f64")
        s.set_data(X, y)
    else:
        s = R.Solver(n, 3, wf, loss, reg=0.01, wstep=2, args=args, B=B, tol=0.0, storage="f64", share=share)
        s.set_labels(labels)
    assert s.risk_path() == 0
    m0 = F.pattern("gaussian", n, wf, args, seed=99)
    s.set_state(w=np.zeros(3), lam=-m0, rho=1.0, iter=1)
    st = s.step()
    return s, int(st.zband)


def _handle(R, monkeypatch, kind, fam, loss, n):
    """the module's handle of (kind, family, loss, n).  kind: "objective_only" (one column, never steps), "sorted"
    (RBL_NO_ZBAND=1, one step), "select" (RBL_ZBAND_MIN_N=16, one step: stats.zband 1 or 2)"""
    key = (kind, fam, loss, n)
    if key not in HANDLES:
        if kind == "objective_only":
            wf, args, _ = F.family(fam, n)
            HANDLES[key] = _one_column(R, fam, loss, F.pattern("gaussian", n, wf, args, seed=98))
        else:
            s, mode = _stepped(R, monkeypatch, kind, fam, loss, n)
            HANDLES[key] = s
            if kind == "select":
                assert mode in (1, 2), (fam, loss, n, "the first step did not take the sort-free z-step", mode)
            else:
                assert mode == 0, (fam, loss, n, mode)
    return HANDLES[key]


def _exact(fam, loss, n, name, case, v, r=None):
    key = (fam, loss, n, name, case, r is not None)
    if key not in REF:
        wf, args, _ = F.family(fam, n)
        REF[key] = F.risk_exact(wf, args, loss, v, r)
    return REF[key]


def _check(label, got, ref, path, want_path):
    err = abs(got - ref) / max(1.0, abs(ref))
    print(f"{label}: got={got:.17g} exact={ref:.17g} err={err:.2e} risk_path={path}")
    assert math.isfinite(got), (label, got)
    assert err <= F.BAR, (label, got, ref, err)
    assert path == want_path, (label, path, want_path)


def _run_patterns(path_id, want_path, fam, n, losses_handles, names=F.PATTERNS, r=None):
    """every case of every pattern at this size through risk_from_v of the handles {loss: solver}.  r: the handles are
    relabelled (r = y_own * y_owner): the pattern is what the handle's losses are taken at, v = r * pattern goes in"""
    wf, args, _ = F.family(fam, n)
    for name, case in F.cases(n, wf, args, names):
        u = F.pattern(name, n, wf, args, seed=5, case=case)
        v = u if r is None else r * u
        dev = _device(v)
        for loss, h in losses_handles.items():
            got = h.risk_from_v(dev.data_ptr())
            _check(f"{path_id} {fam} {loss[:6]} n={n} {name}/{case}", got, _exact(fam, loss, n, name, case, v, r),
                   h.risk_path(), want_path)


def _objective_on_fresh_handles(R, path_id, want_path, fam, n):
    """rbl_objective (w = [1], no regulariser) on one-column problems built from the patterns themselves"""
    wf, args, _ = F.family(fam, n)
    rng = np.random.default_rng([n, 41])
    y = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    for name in OBJECTIVE_PATTERNS:
        v = F.pattern(name, n, wf, args, seed=5)
        for loss in F.losses_of(fam):
            s = _one_column(R, fam, loss, v, y)
            try:
                assert s.risk_path() == 0
                got = s.objective(np.ones(1))
                _check(f"{path_id} objective {fam} {loss[:6]} n={n} {name}", got, _exact(fam, loss, n, name, 0, v),
                       s.risk_path(), want_path)
            finally:
                s.close()


def _fam_n(fams):
    return [(f, n) for f in fams for n in F.SIZES]


def _ids(cases):
    return ["-".join(str(x) for x in c) for c in cases]


# ------------------------------------------------------------------------------------------------------- path A
@pytest.mark.parametrize("n", F.SIZES)
def test_mean_path_erm(R, monkeypatch, n):
    hs = {loss: _handle(R, monkeypatch, "objective_only", "erm", loss, n) for loss in F.LOSSES}
    _run_patterns("A", 1, "erm", n, hs)
    _objective_on_fresh_handles(R, "A", 1, "erm", n)


# ------------------------------------------------------------------------------------------------------- path B
@pytest.mark.parametrize("fam,n", _fam_n(F.SMOOTH), ids=_ids(_fam_n(F.SMOOTH)))
def test_sort_path_smooth_families(R, monkeypatch, fam, n):
    """(`extremes` puts one loss of 1e6 / 1e12 on the last rank, so its error is that of sigma_{n-1} alone: esrm's
    difference of two exponentials cancels to about n eps in the library and in oracle/weights.py alike - measured
    6.7e-13 at n = 4099, the largest error of the file; every other case stays below 1e-15)"""
    hs = {loss: _handle(R, monkeypatch, "objective_only", fam, loss, n) for loss in F.losses_of(fam)}
    _run_patterns("B", 2, fam, n, hs)
    _objective_on_fresh_handles(R, "B", 2, fam, n)


@pytest.mark.parametrize("fam,n", _fam_n(F.BANDED), ids=_ids(_fam_n(F.BANDED)))
def test_sort_path_banded_families_without_the_select(R, monkeypatch, fam, n):
    """RBL_NO_ZBAND=1: the handle has stepped, its weights are banded, and its risk still sorts"""
    hs = {loss: _handle(R, monkeypatch, "sorted", fam, loss, n) for loss in F.LOSSES}
    _run_patterns("B no-zband", 2, fam, n, hs)


@pytest.mark.parametrize("fam,n", _fam_n(F.BANDED), ids=_ids(_fam_n(F.BANDED)))
def test_sort_path_banded_families_on_an_objective_only_handle(R, monkeypatch, fam, n):
    """no z-step ever classifies sigma on such a handle (nor on any handle before its first step): the risk sorts,
    whatever the environment says"""
    _setenv(monkeypatch, "select")
    hs = {loss: _handle(R, monkeypatch, "objective_only", fam, loss, n) for loss in F.LOSSES}
    _run_patterns("B objective-only", 2, fam, n, hs)
    _objective_on_fresh_handles(R, "B objective-only", 2, fam, n)


# ------------------------------------------------------------------------------------------------------- path C
@pytest.mark.parametrize("fam,n", _fam_n(F.BANDED), ids=_ids(_fam_n(F.BANDED)))
def test_select_path_on_every_pattern(R, monkeypatch, fam, n):
    """the sort-free risk on keys tied with, before, behind and across every band edge; a NaN here means the risk-mode
    select reported a status other than OK"""
    hs = {loss: _handle(R, monkeypatch, "select", fam, loss, n) for loss in F.LOSSES}
    _run_patterns("C", 3, fam, n, hs)


@pytest.mark.parametrize("fam", F.BANDED)
def test_sorted_and_select_agree_on_gaussian(R, monkeypatch, fam):
    for n in F.SIZES:
        wf, args, _ = F.family(fam, n)
        dev = _device(F.pattern("gaussian", n, wf, args, seed=6))
        for loss in F.LOSSES:
            b, c = _handle(R, monkeypatch, "sorted", fam, loss, n), _handle(R, monkeypatch, "select", fam, loss, n)
            vb, vc = b.risk_from_v(dev.data_ptr()), c.risk_from_v(dev.data_ptr())
            print(f"B/C {fam} {loss[:6]} n={n}: sorted={vb:.17g} select={vc:.17g} rel={abs(vb - vc) / abs(vb):.2e} "
                  f"risk_path={b.risk_path()}/{c.risk_path()}")
            assert (b.risk_path(), c.risk_path()) == (2, 3)
            assert abs(vb - vc) <= 1e-13 * abs(vb), (fam, loss, n, vb, vc)


# ------------------------------------------------------------------------------------------------------- path D
@pytest.mark.parametrize("loss,n", [(l, n) for l in F.LOSSES for n in F.SIZES],
                         ids=_ids([(l[:6], n) for l in F.LOSSES for n in F.SIZES]))
def test_relabelled_borrowers(R, monkeypatch, loss, n):
    """a borrower with labels y_k on an owner's (X, y): risk_from_v takes v in the OWNER's convention, the losses are
    taken at r * v, r = y_k * y (the RS instances of k_loss_sum and k_loss_keys; the select sees the flipped keys)"""
    X, y = Z.make_problem(n)
    yk = F.relabel(y, seed=n)
    r = yk * y
    assert 0 < np.count_nonzero(r < 0) < n
    owner = R.Solver(n, 3, "erm", loss, reg=0.01, wstep=2, tol=0.0, storage="f64")
    made = [owner]
    try:
        owner.set_data(X, y)
        owner.gram()
        for path_id, want, kind, fams in (("D/A", 1, None, ["erm"]), ("D/B", 2, "sorted", ["extremile", "superq_0.37"]),
                                          ("D/C", 3, "select", F.BANDED)):
            for fam in fams:
                if kind is None:
                    wf, args, B = F.family(fam, n)
                    s = R.Solver(n, 3, wf, loss, reg=0.01, wstep=2, tol=0.0, storage="f64", share=owner)
                    s.set_labels(yk)
                else:
                    s, mode = _stepped(R, monkeypatch, kind, fam, loss, n, share=owner, labels=yk)
                    assert mode in (1, 2) if kind == "select" else mode == 0, (fam, mode)
                made.append(s)
                assert np.array_equal(s.labels(), yk)
                _run_patterns(path_id, want, fam, n, {loss: s}, RELABELLED_PATTERNS, r=r)
    finally:
        for s in reversed(made):
            s.close()


# ------------------------------------------------------------------------------------------------------- path E
SHARDED = [(fam, loss, n, world) for fam in ("superq_0.37", "extremile") for loss in (F.BCE, F.HINGE) for n in (1000, 4099)
           for world in (2, 4)]


@pytest.mark.parametrize("fam,loss,n,world", SHARDED, ids=_ids([(f, l[:6], n, w) for f, l, n, w in SHARDED]))
def test_row_sharded_risk(R, monkeypatch, fam, loss, n, world):
    """each rank's shard of v written into its buf("v"), ShardedADMM._risk_distributed() on the thread hub of
    tests/zstep_inject.py (4099 rows: shards of 2050 / 2049 and 1025 / 1025 / 1025 / 1024)"""
    import torch
    import admm_for_rank_based_loss_amd as rbl
    from admm_for_rank_based_loss_amd import dist as _d  # noqa: F401  (imports finish before the rank threads start)
    rbl._lib.load()
    assert Z.family(fam, n)[:2] == F.family(fam, n)[:2]
    _setenv(monkeypatch, "sorted")
    wf, args, _ = F.family(fam, n)
    cs = F.cases(n, wf, args, SHARDED_PATTERNS)
    vs = [F.pattern(name, n, wf, args, seed=7, case=case) for name, case in cs]

    def body(rk, drv):
        e = rk.engine
        drv.rec = {}                         # (the hub's driver notes which z-step ran)
        drv.step(True)                       # one iteration with its logged objective: v = D w is current and stays so
        view, out = e.buf("v"), []
        assert view.numel() == rk.cnt
        for v in vs:
            view.copy_(torch.from_numpy(v[rk.lo:rk.lo + rk.cnt]))
            rk.sync()
            out.append(drv._risk_distributed())
        return out

    res = Z.run_ranks(Z.GpuRank, fam, loss, n, world, False, body, what="sharded risk")
    for k, (name, case) in enumerate(cs):
        got = [res[rank][k] for rank in range(world)]
        assert len(set(got)) == 1, (name, case, got)                 # one all-reduce: the same bits on every rank
        _check(f"E w{world} {fam} {loss[:6]} n={n} {name}/{case}", got[0], _exact(fam, loss, n, name, ("E", case), vs[k]),
               "-", "-")


# --------------------------------------------------------------------------------------------- accuracy, fairness
STAT_SIZES = [17, 1000, 70001]


def _score_handle(R, loss, xw, y):
    n = xw.size
    s = R.Solver(n, 1, "erm", loss, storage="f64", objective_only=True)
    s.set_data(xw.reshape(n, 1), y)
    return s


def _borrower(R, owner, loss, yk):
    s = R.Solver(owner.n, 1, "erm", loss, storage="f64", objective_only=True, share=owner)
    s.set_labels(yk)
    return s


@pytest.mark.parametrize("n", STAT_SIZES)
def test_accuracy_is_the_reference_count(R, n):
    """rbl_accuracy on fp64 scores is EQUAL to calculate_acc.py:3-19 restated on the same scores: BCE at three
    thresholds (x.w = +0.0 and -0.0 under both labels sit exactly on 0.5 and predict +1), the squared hinge, the hinge
    (the fraction of y = +1), and the same on a relabelled borrower (the RS instance of k_accuracy)"""
    w = np.ones(1)
    for name in F.SCORES:
        xw, y = F.scores(name, n, seed=n)
        yk = F.relabel(y, seed=n)
        for loss in F.LOSSES:
            own = _score_handle(R, loss, xw, y)
            bor = _borrower(R, own, loss, yk)
            try:
                for thr in (F.THRESHOLDS if loss == F.BCE else [0.5]):
                    for what, h, labels in (("own", own, y), ("relabelled", bor, yk)):
                        got, ref = h.accuracy(w, thr), F.accuracy_ref(xw, labels, thr, loss)
                        print(f"accuracy {name} {loss[:6]} n={n} thr={thr} {what}: got={got:.17g} ref={ref:.17g}")
                        assert got == ref, (name, loss, n, thr, what, got, ref)
                        if loss == F.HINGE:
                            assert ref == np.mean(labels == 1.0)
            finally:
                bor.close()
                own.close()


def _same(got, ref, rel):
    if math.isnan(ref):
        return math.isnan(got)
    if math.isinf(ref):
        return got == ref
    return abs(got - ref) <= rel * abs(ref)


@pytest.mark.parametrize("n", STAT_SIZES)
def test_fair_statistics_are_the_reference_counts(R, n):
    """rbl_fair_statistics against fair_metric.py:3-41 restated on the same scores: SPD, DI, EOD, AOD, FNRD (counts) to
    1e-14 relative, the Theil index (fsum of b and b log b) to 1e-12.  Probabilities exactly on the threshold 0.5
    predict +1; group values other than 0 / 1 are in neither group's counts and stay in the Theil sums (the reference's
    masks group == 0 / group == 1 and its sums over all rows do the same); an empty group gives the inf / nan of the
    same divisions; a relabelled borrower (the RS instance of k_fair_counts) is held to the reference on its own labels"""
    w = np.ones(1)
    for name in ("gaussian", "on_threshold"):
        xw, y = F.scores(name, n, seed=n + 1)
        yk = F.relabel(y, seed=n + 1)
        own = _score_handle(R, F.BCE, xw, y)
        bor = _borrower(R, own, F.BCE, yk)
        try:
            for gname in F.GROUPS:
                grp = F.groups(gname, n, seed=n)
                for thr in ([0.5, 0.3] if name == "gaussian" else [0.5]):
                    for what, h, labels in (("own", own, y), ("relabelled", bor, yk)):
                        got, ref = h.fair_statistics(w, grp, thr), F.fair_ref(xw, labels, grp, thr)
                        print(f"fair {name} {gname} n={n} thr={thr} {what}:\n   got={got}\n   ref={ref}")
                        for k, rel in enumerate((1e-14, 1e-14, 1e-14, 1e-14, 1e-12, 1e-14)):
                            assert _same(got[k], ref[k], rel), (name, gname, n, thr, what, k, got[k], ref[k])
                        if gname in ("no_group0", "no_group1"):
                            assert math.isnan(ref[0]) and math.isfinite(ref[4])
                        else:
                            assert all(math.isfinite(x) for x in ref)
        finally:
            bor.close()
            own.close()
