"""Groups of problems on one data matrix (include/rbl.h: rbl_create_shared, rbl_group_*, rbl_k_*_multi) on the GPU:
the multi-column passes against NumPy and against the single-column passes, group iterates against the CPU oracle
member by member, group against standalone, the pass counters, uneven stopping, the sharing of D and G, and the
class API (ADMMgroup)."""
import contextlib
import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

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


# every family of test_gpu_solver.py::test_iterates_match_oracle_exact, plus one sADMM member
MEMBERS = [
    dict(weight_function="erm", loss="binary_cross_entropy", l1_reg=0.01),
    dict(weight_function="erm", loss="hinge", l2_reg=0.01),
    dict(weight_function="superquantile", loss="binary_cross_entropy", l2_reg=0.01, args=[0.5]),
    dict(weight_function="extremile", loss="binary_cross_entropy", l1_reg=0.01, args=[2.0]),
    dict(weight_function="esrm", loss="hinge", l2_reg=0.01, args=[1.0]),
    dict(weight_function="aorr", loss="hinge", l2_reg=1e-4, args=[0.2, 0.8]),
    dict(weight_function="aorr", loss="binary_cross_entropy", l2_reg=1e-4, args=[0.2, 0.8]),
    dict(weight_function="aorr_dc", loss="binary_cross_entropy", l2_reg=1e-4, args=[300, 40]),
    dict(weight_function="ehrm", loss="binary_cross_entropy", l2_reg=0.01, B=-5),
    dict(weight_function="erm", loss="binary_cross_entropy", l1_reg=0.01, smooth=True, t=1.0),
]


def _make(R, X, y, pr, storage, nit, tol=0.0, share=None, no_fuse=False):
    pr = dict(pr)
    smooth = pr.pop("smooth", False)
    if no_fuse:
        os.environ["RBL_NO_FUSE"] = "1"       # read by rbl_create: the two-pass structure for a standalone erm handle
    try:
        if smooth:
            return R.smoothADMMmethod(X, y, max_iter=nit, tol=tol, storage=storage, share_data=share, **pr)
        pr.pop("t", None)
        return R.ADMMmethod(X, y, max_iter=nit, tol=tol, storage=storage, share_data=share, **pr)
    finally:
        os.environ.pop("RBL_NO_FUSE", None)


def _make_group(R, X, y, members, storage, nit, tol=0.0):
    solvers = []
    for pr in members:
        solvers.append(_make(R, X, y, pr, storage, nit, tol, share=solvers[0] if solvers else None))
    return solvers, R._solver.Group([s._s for s in solvers])


def _redone(st):
    """z-steps of this iteration that were not certified and redone: the banded path (zband == 2) or the 32-bit-key
    sort (4 + 8 radix passes)"""
    return int(st.zband == 2) + int(st.sort_passes == 12)


# --------------------------------------------------------------------------------------------------- 1. kernels
@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_multi_column_passes(R, storage):
    """column j of V = D [w_1 .. w_k] / Q = D^T [c_1 .. c_k] against NumPy with the bound of the single-column kernel
    tests (test_gpu_kernels.py::test_gemv_gemvt: 1e-13 x the absolute sum + 1), and against the single-column call."""
    L = R._lib
    rng = np.random.default_rng(11)
    shapes = [(1, 24), (63, 130), (4099, 130), (63, 1000), (4099, 1000), (1, 1001), (63, 1001), (4099, 1001),
              (63, 2048), (700, 2048), (63, 2500), (4099, 160), (300, 24)]
    ks = [1, 2, 3, 5, 8, 11]
    for i, (n, d) in enumerate(shapes):
        D = rng.standard_normal((n, d))
        if storage == "f32":
            D = D.astype(np.float32).astype(np.float64)      # compare on exactly representable data
        for k in (ks if (n, d) in ((4099, 1000), (63, 1001), (4099, 130)) else [ks[i % len(ks)], ks[(i + 3) % len(ks)]]):
            W = rng.standard_normal((k, d))
            Cm = rng.standard_normal((k, n))
            V = L.k_gemv_multi(D, W, storage)
            Q = L.k_gemvt_multi(D, Cm, storage)
            bv = 1e-13 * np.max(np.abs(D) @ np.abs(W.T) + 1, axis=0)
            bq = 1e-13 * np.max(np.abs(D.T) @ np.abs(Cm.T) + 1, axis=0)
            ev = np.max(np.abs(V - (D @ W.T).T), axis=1)
            eq = np.max(np.abs(Q - (D.T @ Cm.T).T), axis=1)
            print(f"multi {storage} n={n} d={d} k={k}: max err V {ev.max():.2e} (bound {bv.min():.2e}) Q {eq.max():.2e} "
                  f"(bound {bq.min():.2e})")
            assert np.all(ev <= bv), (n, d, k, ev, bv)
            assert np.all(eq <= bq), (n, d, k, eq, bq)
            for j in {0, k - 1}:
                v1 = L.k_gemv(D, W[j], storage)
                q1 = L.k_gemvt(D, Cm[j], storage)
                assert np.max(np.abs(V[j] - v1)) <= bv[j], (n, d, k, j)
                assert np.max(np.abs(Q[j] - q1)) <= bq[j], (n, d, k, j)
            # bit-reproducible from run to run
            assert np.array_equal(L.k_gemv_multi(D, W, storage), V)
            assert np.array_equal(L.k_gemvt_multi(D, Cm, storage), Q)


# ------------------------------------------------------------------------------- 2. iterates against the oracle
@pytest.mark.parametrize("n,d,seed,storage,nit", [(1500, 24, 77, "f64", 25), (3000, 160, 5, "f64", 12),
                                                  (2000, 1000, 9, "f32", 6)],
                         ids=["1500x24_own_passes", "3000x160_f64_shared", "2000x1000_f32_shared"])
def test_group_iterates_match_oracle_exact(R, n, d, seed, storage, nit):
    """every member, every iteration: rho, primal, dual, objective, EHRM branch, and the final w, z, lambda against
    oracle.admm.admm_solve(mode="exact") at the tolerances of test_gpu_solver.py::test_iterates_match_oracle_exact
    (1e-9 BCE, 1e-7 hinge; the sADMM member at test_sadmm_iterates_match_oracle_exact's 1e-8 / 1e-7)."""
    from oracle import problems, admm
    X, y = problems.make_problem(n, d, seed=seed)
    if storage == "f32":
        X = X.astype(np.float32).astype(np.float64)     # what the device stores: the oracle sees the same D
    members = [dict(m) for m in MEMBERS]
    if d >= 1000:       # the oracle's exact mode is slow at this width: six members, every kind of z-step and w-step
        members = [members[k] for k in (0, 2, 4, 6, 8, 9)]
    solvers, g = _make_group(R, X, y, members, storage, nit)
    refs = []
    for pr in members:
        kw = {k: v for k, v in pr.items() if k not in ("smooth", "t")}
        extra = dict(smooth=True, t=pr["t"]) if pr.get("smooth") else {}
        refs.append(admm.admm_solve(X, y, max_iter=nit, mode="exact", tol=0.0, **kw, **extra))
    shared = g.counters()["k_per_pass"] >= 2
    assert shared == (d > 64)
    for i in range(nit):
        stats = g.step(want_objective=True)
        for k, (pr, st, ref) in enumerate(zip(members, stats, refs)):
            tol = 1e-9 if pr["loss"] == "binary_cross_entropy" else 1e-7
            if pr.get("smooth"):
                tol = 1e-8
            assert st.iter == i + 1 and st.fused == 0
            assert abs(st.rho - ref.rho[i]) <= 1e-15 * ref.rho[i], (k, i)
            assert abs(st.primal - ref.primal[i]) <= tol * max(1.0, ref.primal[i]), (k, i, st.primal, ref.primal[i])
            assert abs(st.dual - ref.dual[i]) <= tol * max(1.0, ref.dual[i]), (k, i, st.dual, ref.dual[i])
            assert abs(st.objective - ref.objective[i + 1]) <= tol * max(1.0, abs(ref.objective[i + 1])), (k, i)
            if pr["weight_function"] == "ehrm":
                assert st.ehrm_branch == (0 if ref.branch[i] == "a" else 1), (k, i)
            assert st.fused_v == (1 if shared else 0)
    for k, (pr, s, ref) in enumerate(zip(members, solvers, refs)):
        tol = 1e-9 if pr["loss"] == "binary_cross_entropy" else 1e-7
        ztol = 10 * tol
        if pr.get("smooth"):
            tol, ztol = 1e-8, 1e-7
        state = s._s.get_state()
        if pr.get("smooth"):
            assert abs(s.t - ref.t) <= 1e-12 * ref.t
            s._s.finalize_smooth()
            w = s._s.get_state()["w"]
        else:
            w = state["w"]
        assert np.max(np.abs(w - ref.w)) <= tol * max(1.0, np.max(np.abs(ref.w))), k
        assert np.max(np.abs(state["z"] - ref.z)) <= ztol * max(1.0, np.max(np.abs(ref.z))), k
        assert np.max(np.abs(state["lam"] - ref.lam)) <= ztol * max(1e-3, np.max(np.abs(ref.lam))), k
    g.close()


# ------------------------------------------------------------------------- 3. + 4. group = standalone, counters
@pytest.mark.parametrize("n,d,storage", [(3000, 160, "f64"), (5000, 1000, "f32")], ids=["3000x160_f64", "5000x1000_f32"])
def test_group_equals_standalone_and_passes_are_shared(R, n, d, storage):
    """the members stepped alone (erm without the single-sweep pass): w and lambda agree to the bound
    test_gpu_widths.py uses for "same maths, different order of the fp64 sums" (1e-11 relative) - column k of a shared
    pass repeats the single-column pass' order of sums, so rank-weighted members are in fact bit-identical; a repeated
    group run is bit-identical; shared_v == shared_q == nit * ceil(K / k_per_pass); a member's own n x d launches are
    its first v = D w plus one q per redone z-step.  (5000 rows: the sort-free banded z-step runs from iteration 1 on.)
    Host waits: a member of the group waits at least once less per iteration than the same member alone (whose
    rbl_step ends in a wait of its own on the statistics) - except the first member, on which the group's one wait is
    booked.  The standalone runs keep the group's handles alive, so both sides run the same form of the w-step (wstep.hip
    chooses it by the number of live handles)."""
    from oracle import problems
    X, y = problems.make_problem(n, d, seed=100 + d)
    nit = 10
    members = [m for m in MEMBERS if not m.get("smooth")]
    K = len(members)

    def run_group():
        solvers, g = _make_group(R, X, y, members, storage, nit)
        redone = np.zeros((nit, K), dtype=int)
        single, syncs = [], []
        for i in range(nit):
            stats = g.step(want_objective=False)
            redone[i] = [_redone(st) for st in stats]
            single.append(np.array(g.counters()["single_passes"]))
            syncs.append([st.host_syncs for st in stats])
        cnt = g.counters()
        states = [s._s.get_state() for s in solvers]
        g.close()
        return cnt, states, redone, np.array(single), np.array(syncs), solvers

    cnt, states, redone, single, gsyncs, keep = run_group()
    assert np.all(gsyncs[:, 0] >= 1)
    kpp = cnt["k_per_pass"]
    assert kpp >= 2
    assert cnt["shared_v"] == cnt["shared_q"] == nit * -(-K // kpp), cnt
    # iteration 0: every member forms its first v = D w on its own; afterwards only redone z-steps cost a pass
    assert list(single[0]) == [1 + r for r in redone[0]], (single[0], redone[0])
    assert np.array_equal(single[-1] - single[0], redone[1:].sum(axis=0)), (single, redone)
    print("redone z-steps per member:", redone.sum(axis=0).tolist(), "single passes:", single[-1].tolist())
    cnt2, states2, _, _, _, keep2 = run_group()
    del keep2
    for a, b in zip(states, states2):
        for key in ("w", "z", "lam"):
            assert np.array_equal(a[key], b[key]), key
        assert a["rho"] == b["rho"]
    for k, pr in enumerate(members):
        s = _make(R, X, y, pr, storage, nit, no_fuse=pr["weight_function"] == "erm")
        asyncs = 0
        for _ in range(nit):
            st = s._s.step(False)
            assert st.fused == 0
            asyncs += st.host_syncs
        alone = s._s.get_state()
        print(f"member {k}: host waits over {nit} iterations: group {gsyncs[:, k].sum()} alone {asyncs}")
        if k > 0 and pr["weight_function"] != "erm":       # (same trajectory bit for bit: the same w-step waits)
            assert gsyncs[:, k].sum() <= asyncs - nit, (k, gsyncs[:, k].tolist(), asyncs)
        dl = np.max(np.abs(states[k]["lam"] - alone["lam"])) / max(1e-3, np.max(np.abs(alone["lam"])))
        dw = np.max(np.abs(states[k]["w"] - alone["w"])) / max(1.0, np.max(np.abs(alone["w"])))
        print(f"member {k} {pr['weight_function']}/{pr['loss']}: group vs standalone rel lam {dl:.2e} w {dw:.2e}")
        assert dl <= 1e-11 and dw <= 1e-11, (k, pr, dl, dw)
        if pr["weight_function"] != "erm":      # same kernels' order of sums: bit for bit
            assert np.array_equal(states[k]["lam"], alone["lam"]) and np.array_equal(states[k]["w"], alone["w"]), k
        s._s.close()


def test_group_outside_the_shared_widths_runs_member_passes(R):
    from oracle import problems, admm
    X, y = problems.make_problem(1200, 2100, seed=3)
    X = X.astype(np.float32).astype(np.float64)
    members = [MEMBERS[2], MEMBERS[1], MEMBERS[6]]
    nit = 5
    solvers, g = _make_group(R, X, y, members, "f32", nit)
    for _ in range(nit):
        g.step(True)
    cnt = g.counters()
    assert cnt["k_per_pass"] == 1 and cnt["shared_v"] == 0 and cnt["shared_q"] == 0, cnt
    assert all(c >= 2 * nit for c in cnt["single_passes"]), cnt
    for pr, s in zip(members, solvers):
        ref = admm.admm_solve(X, y, max_iter=nit, mode="exact", tol=0.0, **pr)
        tol = 1e-9 if pr["loss"] == "binary_cross_entropy" else 1e-7
        assert np.max(np.abs(s._s.get_state()["w"] - ref.w)) <= tol * max(1.0, np.max(np.abs(ref.w)))
    g.close()


# ------------------------------------------------------------------------------------------- 5. uneven stopping
def test_uneven_stopping(R):
    """members with different tol / reg: each stops at the iteration its standalone rbl_solve stops at, with that state;
    later steps leave it untouched bit for bit; the group ends with the last one."""
    from oracle import problems
    X, y = problems.make_problem(3000, 160, seed=21)
    base = dict(weight_function="superquantile", loss="binary_cross_entropy", args=[0.5])
    specs = [(dict(base, l2_reg=0.01), 1e-2), (dict(base, l2_reg=0.1), 1e-3), (dict(base, l2_reg=1.0), 3e-3),
             (dict(weight_function="extremile", loss="binary_cross_entropy", l2_reg=0.05, args=[2.0]), 1e-9),
             (dict(weight_function="erm", loss="binary_cross_entropy", l2_reg=0.5), 2e-3)]
    cap = 120
    # (a second live handle, as in the group: wstep.hip chooses the form of the w-step by the number of live handles)
    keep = R._solver.Solver(64, 8, "erm", reg=0.1, storage="f64")
    alone = []
    for pr, tol in specs:
        s = _make(R, X, y, pr, "f64", cap, tol=tol, no_fuse=pr["weight_function"] == "erm")
        st, _ = s._s.solve(cap)
        alone.append((int(st.iter), int(st.converged), s._s.get_state()))
        s._s.close()
    keep.close()
    iters = [a[0] for a in alone]
    print("standalone stopping iterations:", iters, "converged:", [a[1] for a in alone])
    assert len(set(iters)) >= 3 and any(a[1] for a in alone), iters      # really uneven
    solvers = []
    for pr, tol in specs:
        solvers.append(_make(R, X, y, pr, "f64", cap, tol=tol, share=solvers[0] if solvers else None))
    g = R._solver.Group([s._s for s in solvers])
    frozen = {}
    steps = 0
    while steps < cap:
        stats = g.step(False)
        steps += 1
        for k, st in enumerate(stats):
            if st.converged and k not in frozen:
                frozen[k] = (steps, solvers[k]._s.get_state())
            elif k in frozen:
                now = solvers[k]._s.get_state()
                for key in ("w", "z", "lam"):
                    assert np.array_equal(now[key], frozen[k][1][key]), (k, key, steps)
                assert now["rho"] == frozen[k][1]["rho"] and now["iter"] == frozen[k][1]["iter"]
        if all(st.converged for st in stats):
            break
    assert steps == max(iters), (steps, iters)
    for k, (it, conv, ref) in enumerate(alone):
        now = solvers[k]._s.get_state()
        assert now["iter"] == it, (k, now["iter"], it)
        assert (k in frozen) == bool(conv)
        if conv:
            assert frozen[k][0] == it
        assert np.max(np.abs(now["lam"] - ref["lam"])) <= 1e-11 * max(1e-3, np.max(np.abs(ref["lam"]))), k
        assert np.max(np.abs(now["w"] - ref["w"])) <= 1e-11 * max(1.0, np.max(np.abs(ref["w"]))), k
    g.close()
    # rbl_group_solve: the same end, with per-member histories
    solvers = []
    for pr, tol in specs:
        solvers.append(_make(R, X, y, pr, "f64", cap, tol=tol, share=solvers[0] if solvers else None))
    g = R._solver.Group([s._s for s in solvers])
    last, hist = g.solve(cap)
    assert [int(st.iter) for st in last] == iters
    assert [len(h["primal"]) for h in hist] == iters
    g.close()


# --------------------------------------------------------------------------------------------------- 6. sharing
def test_borrower_alone_is_an_ordinary_handle(R):
    from oracle import problems
    X, y = problems.make_problem(3000, 160, seed=8)
    kw = dict(weight_function="extremile", loss="binary_cross_entropy", l1_reg=0.01, args=[2.0])
    nit = 12
    own = _make(R, X, y, kw, "f32", nit)
    owner = _make(R, X, y, MEMBERS[1], "f32", nit)
    bor = _make(R, X, y, kw, "f32", nit, share=owner)
    assert bor._s.info()["lipschitz"] == owner._s.info()["lipschitz"] == own._s.info()["lipschitz"]
    owner._s.close()                      # the owner goes first: the borrower keeps D and G alive
    del owner
    for _ in range(nit):
        a, b = own._s.step(True), bor._s.step(True)
        assert (a.primal, a.dual, a.objective, a.rho_next) == (b.primal, b.dual, b.objective, b.rho_next)
    sa, sb = own._s.get_state(), bor._s.get_state()
    for key in ("w", "z", "lam"):
        assert np.array_equal(sa[key], sb[key]), key
    assert np.array_equal(own._s.get_D(), bor._s.get_D())
    # the data path belongs to the owner
    L = R._lib
    for call in (lambda: bor._s.set_data(X, y), bor._s.gram, bor._s.gram_local, bor._s.gram_finish, bor._s.generate_synthetic,
                 bor._s.synth_local, bor._s.synth_finish):
        with pytest.raises(L.RblError, match="borrows its data") as e:
            call()
        assert e.value.code == L.RBL_ERR_STATE


def test_create_shared_refuses_mismatches(R):
    S = R._solver.Solver
    L = R._lib
    owner = S(500, 40, "erm", reg=0.1, storage="f32")
    with pytest.raises(L.RblError, match="no data yet") as e:
        S(500, 40, "erm", reg=0.1, storage="f32", share=owner)
    assert e.value.code == L.RBL_ERR_STATE
    owner.generate_synthetic(seed=3)
    with pytest.raises(L.RblError, match="Gram matrix is not ready") as e:
        S(500, 40, "erm", reg=0.1, storage="f32", share=owner)
    assert e.value.code == L.RBL_ERR_STATE
    S(500, 40, "erm", storage="f32", objective_only=True, share=owner).close()    # an objective handle needs D only
    owner.gram()
    for kw in (dict(n=499), dict(d=41), dict(storage="f64"), dict(device=1), dict(n=250, n_total=500),
               dict(n=250, n_total=500, row_offset=250)):
        args = dict(n=500, d=40, storage="f32", device=0)
        args.update(kw)
        with pytest.raises(ValueError, match="disagrees with the owner"):
            S(args.pop("n"), args.pop("d"), "superquantile", reg=0.1, args=[0.5], share=owner, **args)
    b = S(500, 40, "superquantile", reg=0.1, args=[0.5], storage="f32", share=owner)
    other = S(500, 40, "erm", reg=0.1, storage="f32")
    other.generate_synthetic(seed=3)
    with pytest.raises(ValueError, match="does not share member 0's data"):
        R._solver.Group([owner, b, other])
    with pytest.raises(ValueError, match="listed twice"):
        R._solver.Group([owner, b, owner])
    g = R._solver.Group([owner, b])
    with pytest.raises(ValueError, match="already belongs to a group"):
        R._solver.Group([b])
    g.step()
    g.close()
    b.step()                               # usable alone again
    shard = S(250, 40, "erm", reg=0.1, storage="f32", n_total=500)
    with pytest.raises(ValueError, match="row shard"):
        R._solver.Group([shard])


def test_borrowers_cost_little_device_memory(R):
    """200 000 x 1000 fp32: D is 800 MB; a borrower's per-row state is a few dozen to a couple of hundred bytes per row
    against the 4000 of its row of D - asserted below a quarter of D"""
    import torch
    S = R._solver.Solver
    n, d = 200_000, 1000
    dbytes = n * d * 4
    owner = S(n, d, "superquantile", reg=0.01, args=[0.5], storage="f32")
    owner.generate_synthetic(seed=5)
    owner.gram()
    torch.cuda.synchronize()

    def used():
        free, total = torch.cuda.mem_get_info(0)
        return total - free

    u0 = used()
    borrowers = []
    for kw in (dict(weight_function="superquantile", args=[0.9]), dict(weight_function="extremile", args=[2.0]),
               dict(weight_function="erm"), dict(weight_function="ehrm", B=-5)):
        b = S(n, d, reg=0.01, storage="f32", share=owner, **kw)
        u1 = used()
        print(f"borrower {kw['weight_function']}: {(u1 - u0) / 1e6:.1f} MB against D = {dbytes / 1e6:.0f} MB")
        assert u1 - u0 < 0.25 * dbytes, (kw, u1 - u0, dbytes)
        borrowers.append(b)
        u0 = u1
    g = R._solver.Group([owner] + borrowers)
    for _ in range(3):
        stats = g.step(True)
    assert all(np.isfinite(st.objective) for st in stats)
    g.close()


# ------------------------------------------------------------------------------------------------ 7. class API
def test_admmgroup_matches_separate_solvers(R):
    from oracle import problems
    X, y = problems.make_problem(2400, 160, seed=12)
    Xt, yt = problems.make_problem(600, 160, seed=13)
    probs = [dict(weight_function="superquantile", loss="binary_cross_entropy", l2_reg=0.01, args=[q]) for q in (0.3, 0.6, 0.9)]
    probs += [dict(weight_function="aorr", loss="hinge", l2_reg=1e-4, args=[0.2, 0.8]),
              dict(weight_function="erm", loss="binary_cross_entropy", l1_reg=0.01),
              dict(weight_function="erm", loss="binary_cross_entropy", l1_reg=0.01, smooth=True, t=1.0)]
    nit = 15
    grp = R.ADMMgroup(X, y, probs, storage="f64", max_iter=nit, tol=0.0)
    assert [type(s).__name__ for s in grp.solvers] == ["ADMMmethod"] * 5 + ["smoothADMMmethod"]
    grp.start_store(Xt, yt)
    ws = _quiet(grp.main_loop, verbose=False)
    res = grp.final_res()
    cnt = grp.counters()
    assert cnt["shared_v"] == cnt["shared_q"] == nit * -(-len(probs) // cnt["k_per_pass"])
    for k, pr in enumerate(probs):
        pr = dict(pr)
        smooth = pr.pop("smooth", False)
        t = pr.pop("t", 1)
        s = R.smoothADMMmethod(X, y, t=t, max_iter=nit, tol=0.0, storage="f64", **pr) if smooth else \
            R.ADMMmethod(X, y, max_iter=nit, tol=0.0, storage="f64", **pr)
        skw = {k2: v for k2, v in pr.items() if k2 != "w0"}
        s.start_store(Xt, yt, **skw)
        w = _quiet(s.main_loop, verbose=False)
        w1, _, train, test = s.final_res()
        wg, times, gtrain, gtest = res[k]
        # both sides are within tol of the oracle (test_iterates_match_oracle_exact): within 2 tol of each other
        tol = 2 * (1e-9 if pr["loss"] == "binary_cross_entropy" else 1e-7)
        assert len(gtrain) == len(train) == nit + 1 and len(gtest) == len(test) and len(times) == nit + 1
        assert np.allclose(gtrain, train, rtol=tol, atol=tol), (k, np.max(np.abs(np.array(gtrain) - train)))
        assert np.allclose(gtest, test, rtol=tol, atol=tol), k
        assert np.max(np.abs(wg - w1)) <= tol * max(1.0, np.max(np.abs(w1))), k
        assert np.array_equal(ws[k], wg)
        assert grp.solvers[k].objective.get_arrogate_loss(wg) == pytest.approx(s.objective.get_arrogate_loss(w), rel=1e-7)
    grp.close()


# ------------------------------------------------- 8. an uncertified z-step of a member behind the shared passes
# path -> (family of both members, the m the fast path must refuse, environment read at each handle's first z-step)
UNCERTIFIED = {
    "banded": ("superq_0.5", "all_equal", {"RBL_NO_ZBAND": "0", "RBL_NO_SORT32": "0", "RBL_ZBAND_MIN_N": "16"}),
    "sort32": ("extremile", "two_values", {"RBL_NO_ZBAND": "1", "RBL_NO_SORT32": "0"}),
}


@pytest.mark.parametrize("path,storage", [("banded", "f32"), ("sort32", "f32"), ("banded", "csr")])
def test_uncertified_z_step_of_a_member_behind_shared_passes(R, monkeypatch, path, storage):
    """Two rank-weighted members on one X with a prescribed m each (tests/zstep_inject.py: set_state(w = 0,
    lam = -rho m0, rho = 2^-4, iter = 200)): member A's m is benign, member B's is one its fast z-step cannot certify
    (keys tied across the band edge; a run of equal 32-bit keys).  B's q came out of the shared Q pass; its rbl_phase_w
    settles the verdict and redoes z and q for B alone.  Each member's z equals, bit for bit, the z of a handle of its
    own with the same state after rbl_step; the shared passes ran once each; B cost one n x d launch more than A.
    132 columns: the narrowest width the dense multi-column passes take; storage="csr": the opt-in sparse ones."""
    import torch
    import zstep_inject as Z
    fam, bad, env = UNCERTIFIED[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n, d, rho, it = 4096, 132, 2.0 ** -4, 200
    wf, args, B, _, _ = Z.family(fam, n)
    X, y = Z.make_problem(n, d)
    if storage == "csr":
        X = torch.from_numpy(X).to_sparse_csr()          # every entry stored
    m0 = [Z.pattern("gaussian", n, 2, fam), Z.pattern(bad, n, 1, fam)]

    def handle(share=None):
        s = R.Solver(n, d, wf, Z.BCE, reg=0.01, wstep=2, args=args, B=B, tol=0.0, storage=storage, share=share)
        if share is None:
            s.set_data(X, y)
            s.gram()
        return s

    def inject(s, m):
        s.set_state(w=np.zeros(d), lam=-rho * m, rho=rho, iter=it)

    members = [handle()]
    members.append(handle(share=members[0]))
    g = R._solver.Group(members, share_sparse=storage == "csr")
    for s, m in zip(members, m0):
        inject(s, m)
    c0 = g.counters()
    a, b = g.step(False)
    c1 = g.counters()
    zg = [s.get_state(want_lam=False)["z"].copy() for s in members]
    print(f"{path} {storage}: k_per_pass={c0['k_per_pass']} A zband={a.zband} passes={a.sort_passes} "
          f"B zband={b.zband} passes={b.sort_passes} counters {c0} -> {c1}")
    assert c0["k_per_pass"] >= 2 and (storage != "csr" or c0["k_per_pass"] == 4), c0     # the shared passes are on
    if path == "banded":
        assert (a.zband, b.zband) == (1, 2), (a.zband, b.zband)
    else:
        assert (a.zband, a.sort_passes, b.zband, b.sort_passes) == (0, 4, 0, 12), (a.sort_passes, b.sort_passes)
    assert c1["shared_q"] - c0["shared_q"] == 1 and c1["shared_v"] - c0["shared_v"] == 1, (c0, c1)
    own = [c1["single_passes"][k] - c0["single_passes"][k] for k in (0, 1)]
    assert own[1] == own[0] + 1, own                      # the q redone for B alone
    # the group's handles stay alive beside the standalone ones: the same form of the w-step on both sides
    for k, m in enumerate(m0):
        s = handle()
        inject(s, m)
        st = s.step(False)
        z = s.get_state(want_lam=False)["z"]
        s.close()
        assert (st.zband, st.sort_passes) == ((a, b)[k].zband, (a, b)[k].sort_passes), k
        assert np.array_equal(zg[k].view(np.uint64), z.view(np.uint64)), (path, storage, k, float(np.max(np.abs(zg[k] - z))))
    g.close()
    for s in members:
        s.close()


def test_run_group_example():
    env = dict(os.environ, RBL_EXAMPLE_FAST="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_group.py")], capture_output=True, text=True,
                       timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [ln for ln in r.stdout.splitlines() if ln.count(",") >= 5]
    assert len(rows) >= 8, r.stdout
