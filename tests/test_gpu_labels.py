"""Members with labels of their own on one data matrix (include/rbl.h: rbl_set_labels, rbl_decide_multi) on the GPU: a
relabelled borrower - alone and in a group whose members all carry different labels - is bit-identical to a handle
built from (X, y_k); iterates against the CPU oracle; the shared passes cost what equal labels cost; the host-side
entry points speak the member's own sign convention; every refusal; the extra device memory is one byte per row; the
one-vs-rest decision against NumPy; OneVsRest and its example end to end."""
import contextlib
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_group import MEMBERS, _make

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


def _label_vectors(y, K, seed):
    """K label vectors on the rows of y: y itself, then y with a random 30 % of the rows flipped (another draw per
    member).  Both signs occur in every vector and in every r = y_k * y_0 - asserted, not assumed."""
    rng = np.random.default_rng(seed)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    ys = [y.copy()]
    for k in range(1, K):
        ys.append(np.where(rng.random(y.size) < 0.3, -y, y))
    for k, yk in enumerate(ys):
        assert set(np.unique(yk)) == {-1.0, 1.0}, k
        if k > 0:
            assert set(np.unique(yk * ys[0])) == {-1.0, 1.0}, k
            assert all(not np.array_equal(yk, yj) for yj in ys[:k]), k
    return ys


def _is_erm(pr):
    return pr["weight_function"] == "erm"


# ------------------------------------------------------------------------------------------------ 1. bit identity
@pytest.mark.parametrize("storage", ["f32", "f64"])
@pytest.mark.parametrize("d", [24, 160, 1000])
def test_relabelled_member_is_bit_identical_to_standalone(R, d, storage):
    """every family of test_gpu_group.py::MEMBERS, 5000 rows (the sort-free banded z-step runs from iteration 1 on),
    10 iterations.  Member k with labels y_k on the owner's D - stepped alone, and in a group whose members all carry
    different labels - against a handle built from (X, y_k) (erm: RBL_NO_FUSE=1, the two-pass iteration; the group's
    handles stay alive so both sides run the same form of the w-step): w, z, lambda, rho bit for bit, with the same
    z-step path (zband, sort_passes) in every iteration.  erm members inside a group: 1e-11 relative, the bound
    test_gpu_group.py uses for a shared pass against the standalone pass (the order of the sums differs)."""
    from oracle import problems
    n, nit = 5000, 10
    X, y = problems.make_problem(n, d, seed=300 + d)
    if storage == "f32":
        X = X.astype(np.float32).astype(np.float64)
    members = [dict(m) for m in MEMBERS]
    K = len(members)
    ys = _label_vectors(y, K, seed=d)

    # the group: member 0 owns (X, y_0), member k borrows it with labels y_k
    grp = []
    for k, pr in enumerate(members):
        grp.append(_make(R, X, ys[k], pr, storage, nit, share=grp[0] if grp else None))
    g = R._solver.Group([s._s for s in grp])
    gpath = []
    for _ in range(nit):
        stats = g.step(want_objective=False)
        assert all(st.fused == 0 for st in stats)
        gpath.append([(st.zband, st.sort_passes) for st in stats])
    cnt = g.counters()
    assert (cnt["k_per_pass"] >= 2) == (d > 64), cnt
    gstates = [s._s.get_state() for s in grp]
    g.close()

    for k, pr in enumerate(members):
        alone = _make(R, X, ys[k], pr, storage, nit, share=grp[0], no_fuse=_is_erm(pr))      # relabelled borrower, alone
        ref = _make(R, X, ys[k], pr, storage, nit, no_fuse=_is_erm(pr))                      # built from (X, y_k)
        assert np.array_equal(alone._s.labels(), ys[k]) and np.array_equal(ref._s.labels(), ys[k])
        for i in range(nit):
            a, b = alone._s.step(False), ref._s.step(False)
            assert a.fused == 0 and b.fused == 0
            assert (a.zband, a.sort_passes) == (b.zband, b.sort_passes), (k, i)
            assert (a.primal, a.dual, a.rho_next) == (b.primal, b.dual, b.rho_next), (k, i)
            if not _is_erm(pr):
                assert gpath[i][k] == (b.zband, b.sort_passes), (k, i, gpath[i][k])
        sa, sr, sg = alone._s.get_state(), ref._s.get_state(), gstates[k]
        if not _is_erm(pr) and pr["weight_function"] in ("superquantile", "aorr", "aorr_dc"):
            assert any(p[k][0] == 1 for p in gpath), (k, "the banded z-step never ran")
        for key in ("w", "z", "lam"):
            assert np.array_equal(sa[key], sr[key]), (k, pr, key, "alone")
        assert sa["rho"] == sr["rho"] and sa["iter"] == sr["iter"] == nit
        if _is_erm(pr):
            for key, floor in (("w", 1.0), ("z", 1.0), ("lam", 1e-3)):
                rel = np.max(np.abs(sg[key] - sr[key])) / max(floor, np.max(np.abs(sr[key])))
                print(f"d={d} {storage} member {k} erm/{pr['loss']} in the group: rel {key} {rel:.2e}")
                assert rel <= 1e-11, (k, pr, key, rel)
        else:
            for key in ("w", "z", "lam"):
                assert np.array_equal(sg[key], sr[key]), (k, pr, key, "group")
            assert sg["rho"] == sr["rho"]
        alone._s.close()
        ref._s.close()


# --------------------------------------------------------------------------- 2. against the oracle, pass counters
def test_relabelled_group_matches_oracle_and_shares_the_passes(R):
    """every member and iteration against oracle.admm.admm_solve(X, y_k, mode="exact") at the tolerances of
    test_gpu_group.py::test_group_iterates_match_oracle_exact (1e-9 BCE, 1e-7 hinge, 1e-8 sADMM), objective included;
    K members with K different label vectors cost nit * ceil(K / k_per_pass) shared V and Q launches - what K members
    with equal labels cost."""
    from oracle import problems, admm
    n, d, nit, storage = 2000, 160, 8, "f64"
    X, y = problems.make_problem(n, d, seed=41)
    members = [dict(m) for m in MEMBERS]
    K = len(members)
    ys = _label_vectors(y, K, seed=7)
    solvers = []
    for k, pr in enumerate(members):
        solvers.append(_make(R, X, ys[k], pr, storage, nit, share=solvers[0] if solvers else None))
    g = R._solver.Group([s._s for s in solvers])
    refs = []
    for pr, yk in zip(members, ys):
        kw = {k: v for k, v in pr.items() if k not in ("smooth", "t")}
        extra = dict(smooth=True, t=pr["t"]) if pr.get("smooth") else {}
        refs.append(admm.admm_solve(X, yk, max_iter=nit, mode="exact", tol=0.0, **kw, **extra))
    redone = 0
    for i in range(nit):
        stats = g.step(want_objective=True)
        for k, (pr, st, ref) in enumerate(zip(members, stats, refs)):
            tol = 1e-9 if pr["loss"] == "binary_cross_entropy" else 1e-7
            if pr.get("smooth"):
                tol = 1e-8
            assert st.iter == i + 1 and st.fused == 0 and st.fused_v == 1
            assert abs(st.rho - ref.rho[i]) <= 1e-15 * ref.rho[i], (k, i)
            assert abs(st.primal - ref.primal[i]) <= tol * max(1.0, ref.primal[i]), (k, i, st.primal, ref.primal[i])
            assert abs(st.dual - ref.dual[i]) <= tol * max(1.0, ref.dual[i]), (k, i, st.dual, ref.dual[i])
            assert abs(st.objective - ref.objective[i + 1]) <= tol * max(1.0, abs(ref.objective[i + 1])), \
                (k, i, st.objective, ref.objective[i + 1])
            if pr["weight_function"] == "ehrm":
                assert st.ehrm_branch == (0 if ref.branch[i] == "a" else 1), (k, i)
            redone += int(st.zband == 2) + int(st.sort_passes == 12)
    cnt = g.counters()
    assert cnt["k_per_pass"] >= 2
    assert cnt["shared_v"] == cnt["shared_q"] == nit * -(-K // cnt["k_per_pass"]), cnt
    assert sum(cnt["single_passes"]) == K + redone, (cnt, redone)      # the first v = D w of every member, redone z-steps
    for k, (pr, s, ref) in enumerate(zip(members, solvers, refs)):
        tol = 1e-9 if pr["loss"] == "binary_cross_entropy" else 1e-7
        ztol = 10 * tol
        if pr.get("smooth"):
            tol, ztol = 1e-8, 1e-7
        state = s._s.get_state()
        w = state["w"]
        if pr.get("smooth"):
            s._s.finalize_smooth()
            w = s._s.get_state()["w"]
        assert np.max(np.abs(w - ref.w)) <= tol * max(1.0, np.max(np.abs(ref.w))), k
        assert np.max(np.abs(state["z"] - ref.z)) <= ztol * max(1.0, np.max(np.abs(ref.z))), k
        assert np.max(np.abs(state["lam"] - ref.lam)) <= ztol * max(1e-3, np.max(np.abs(ref.lam))), k
    g.close()


# ------------------------------------------------------------------------- 3. the member's own sign convention
def test_host_entry_points_speak_the_members_convention(R):
    from oracle import problems, admm, weights
    n, d = 3000, 160
    X, y = problems.make_problem(n, d, seed=19)
    yk = _label_vectors(y, 2, seed=3)[1]
    pr = dict(weight_function="superquantile", loss="binary_cross_entropy", l2_reg=0.01, args=[0.5])
    owner = _make(R, X, y, MEMBERS[3], "f64", 20)
    bor = _make(R, X, yk, pr, "f64", 20, share=owner)
    ref = _make(R, X, yk, pr, "f64", 20)
    assert np.array_equal(bor._s.labels(), yk) and np.array_equal(owner._s.labels(), y.reshape(-1))
    assert np.array_equal(bor._s.get_D(), -yk.reshape(-1, 1) * X)
    assert np.array_equal(owner._s.get_D(), -y.reshape(-1, 1) * X)
    s0 = bor._s.get_state()
    assert np.array_equal(s0["z"], np.full(n, 0.1 * 0.01 / n)) and np.array_equal(s0["lam"], s0["z"])   # algorithms.py:32-34
    for _ in range(3):
        bor._s.step(True)
        ref._s.step(True)
    sb, sr = bor._s.get_state(), ref._s.get_state()
    for key in ("w", "z", "lam"):
        assert np.array_equal(sb[key], sr[key]), key
    # set_state round trip: a fresh relabelled borrower continues the trajectory bit for bit
    bor2 = _make(R, X, yk, pr, "f64", 20, share=owner)
    bor2._s.set_state(w=sr["w"], z=sr["z"], lam=sr["lam"], rho=sr["rho"], iter=sr["iter"])
    back = bor2._s.get_state()
    for key in ("w", "z", "lam"):
        assert np.array_equal(back[key], sr[key]), key
    for _ in range(2):
        a, b = bor2._s.step(True), ref._s.step(True)
        assert (a.primal, a.dual, a.objective, a.rho_next) == (b.primal, b.dual, b.objective, b.rho_next)
    sb, sr = bor2._s.get_state(), ref._s.get_state()
    for key in ("w", "z", "lam"):
        assert np.array_equal(sb[key], sr[key]), key
    # the caller's own z-step (the oracle's, in the member's convention) on both handles
    sa, sbeta = weights.get_weights("superquantile", n, [0.5])
    Dk = -yk.reshape(-1, 1) * X
    m = Dk @ sr["w"] - sr["lam"] / sr["rho"]
    z_or, _ = admm.z_step_exact("superquantile", "binary_cross_entropy", sa, sbeta, None, sr["rho"], m)
    lib_step = _make(R, X, yk, pr, "f64", 20, share=owner)
    lib_step._s.set_state(w=sr["w"], z=sr["z"], lam=sr["lam"], rho=sr["rho"], iter=sr["iter"])
    lib_step._s.step(False)
    for h in (bor2._s, ref._s):
        h.phase_z_external(z_or)
        h.phase_q()
        h.phase_w()
        h.phase_dual(False)
        h.phase_finish()
    sb, sr2 = bor2._s.get_state(), ref._s.get_state()
    for key in ("w", "z", "lam"):
        assert np.array_equal(sb[key], sr2[key]), key
    assert np.array_equal(sb["z"], z_or)
    wl = lib_step._s.get_state()["w"]
    assert np.max(np.abs(sb["w"] - wl)) <= 1e-9 * max(1.0, np.max(np.abs(wl)))
    # y equal to the owner's: an ordinary borrower
    same = _make(R, X, y, pr, "f64", 20, share=owner)
    plain = R._solver.Solver(n, d, "superquantile", reg=0.01, args=[0.5], storage="f64", max_iter=20, tol=0.0, share=owner._s)
    for _ in range(3):
        a, b = same._s.step(True), plain.step(True)
        assert (a.primal, a.dual, a.objective) == (b.primal, b.dual, b.objective)
    # an objective-only borrower with test labels of its own
    from oracle import objective as oobj
    Xt, yt = problems.make_problem(900, d, seed=23)
    ytk = _label_vectors(yt, 2, seed=5)[1]
    w = sr["w"]
    for wf, args, loss in (("superquantile", [0.5], "binary_cross_entropy"), ("erm", None, "binary_cross_entropy"),
                           ("extremile", [2.0], "hinge")):
        t_own = R.rankbasedObjective(Xt, yt, wf, loss, args=args, storage="f64")
        t_bor = R.rankbasedObjective(Xt, ytk, wf, loss, args=args, storage="f64", _share_data=t_own)
        al, _ = weights.get_weights(wf, 900, args)
        want = oobj.objective(loss, al, Xt, ytk, w, include_reg=False)
        got = t_bor.get_arrogate_loss(w, include_reg=False)
        assert abs(got - want) <= 1e-10 * max(1.0, abs(want)), (wf, got, want)
        assert np.array_equal(t_bor._s.labels(), ytk)
        if loss == "binary_cross_entropy":
            acc = np.mean(np.where(Xt @ w >= 0.0, 1.0, -1.0) == ytk)
            assert t_bor._s.accuracy(w) == pytest.approx(acc, abs=1e-12)
            acc0 = np.mean(np.where(Xt @ w >= 0.0, 1.0, -1.0) == yt.reshape(-1))
            assert t_own._s.accuracy(w) == pytest.approx(acc0, abs=1e-12)
            assert acc != acc0


def test_set_labels_refusals(R):
    L = R._lib
    S = R._solver.Solver
    n, d = 500, 40
    owner = S(n, d, "superquantile", reg=0.1, args=[0.5], storage="f32")
    owner.generate_synthetic(seed=3)
    owner.gram()
    y0 = owner.labels()
    yk = _label_vectors(y0, 2, seed=1)[1]
    with pytest.raises(L.RblError, match="borrows its data") as e:          # the owner
        owner.set_labels(yk)
    assert e.value.code == L.RBL_ERR_STATE
    b = S(n, d, "superquantile", reg=0.1, args=[0.5], storage="f32", share=owner)
    bad = yk.copy()
    bad[7] = 0.25
    assert L.load().rbl_set_labels(b._h, L.ptr(bad)) == L.RBL_ERR_INVALID   # a value other than +-1 (past the Python check)
    assert "labels must be +1/-1" in L.last_error()
    b.set_labels(yk)
    b.set_labels(-yk)                                                        # before the first iteration: as often as wanted
    assert np.array_equal(b.labels(), -yk)
    b.set_labels(yk)
    g = R._solver.Group([owner, b])
    with pytest.raises(L.RblError, match="member of a group") as e:         # inside a group
        b.set_labels(yk)
    assert e.value.code == L.RBL_ERR_STATE
    g.close()
    b.step()
    with pytest.raises(L.RblError, match="has iterated already") as e:      # after a step
        b.set_labels(yk)
    assert e.value.code == L.RBL_ERR_STATE
    assert np.array_equal(b.labels(), yk)
    # a row shard
    so = S(250, d, "superquantile", reg=0.1, args=[0.5], storage="f32", n_total=500)
    so.synth_local(seed=3)
    so.synth_finish()
    so.gram_local()
    so.gram_finish()
    sb = S(250, d, "superquantile", reg=0.1, args=[0.5], storage="f32", n_total=500, share=so)
    with pytest.raises(ValueError, match="row-sharded"):
        sb.set_labels(-so.labels())


# --------------------------------------------------------------------------------------------------- 4. memory
def test_relabelled_borrower_costs_one_byte_per_row(R):
    """method of test_gpu_group.py::test_borrowers_cost_little_device_memory: a borrower with labels of its own against
    an ordinary borrower of the same problem - the sign vector, one byte per row, plus the granularity of one device
    allocation (2 MiB pages)."""
    import torch
    S = R._solver.Solver
    n, d = 400_000, 160
    owner = S(n, d, "superquantile", reg=0.01, args=[0.5], storage="f32")
    owner.generate_synthetic(seed=5)
    owner.gram()
    yk = _label_vectors(owner.labels(), 2, seed=9)[1]
    torch.cuda.synchronize()

    def used():
        free, total = torch.cuda.mem_get_info(0)
        return total - free

    u0 = used()
    plain = S(n, d, "superquantile", reg=0.01, args=[0.9], storage="f32", share=owner)
    u1 = used()
    rel = S(n, d, "superquantile", reg=0.01, args=[0.9], storage="f32", share=owner)
    rel.set_labels(yk)
    u2 = used()
    print(f"ordinary borrower {(u1 - u0) / 1e6:.2f} MB, with labels of its own {(u2 - u1) / 1e6:.2f} MB, n = {n}")
    assert (u2 - u1) - (u1 - u0) <= n + (2 << 20), (u0, u1, u2)
    for _ in range(3):
        st = rel.step(True)
    assert np.isfinite(st.objective)


# ------------------------------------------------------------------------------------------ 5. one-vs-rest decision
@pytest.mark.parametrize("storage", ["f32", "f64"])
def test_decide_multi_against_numpy(R, storage):
    """argmax_j x_i . w_j at the shapes of test_gpu_group.py::test_multi_column_passes on exactly representable data.
    Rows whose two best NumPy scores are closer than that test's bound, 1e-13 (|x_i| . |w_j| + 1), are left out - never
    more than 1 % of a case's rows (with Gaussian W none are)."""
    S = R._solver.Solver
    rng = np.random.default_rng(13)
    shapes = [(1, 24), (63, 130), (4099, 130), (63, 1000), (4099, 1000), (1, 1001), (63, 1001), (4099, 1001),
              (63, 2048), (700, 2048), (63, 2500), (4099, 160), (300, 24)]
    for n, d in shapes:
        X = rng.standard_normal((n, d))
        if storage == "f32":
            X = X.astype(np.float32).astype(np.float64)
        y = np.where(rng.random(n) < 0.5, -1.0, 1.0)           # D = -y X: the decision takes the sign out again
        data = S(n, d, "erm", storage=storage, objective_only=True)
        data.set_data(X, y)
        for k in (1, 2, 3, 5, 8):
            W = rng.standard_normal((k, d))
            cls = data.decide_multi(W)
            assert cls.dtype == np.int32 and cls.shape == (n,)
            sc = X @ W.T
            want = np.argmax(sc, axis=1)
            keep = np.ones(n, dtype=bool)
            if k > 1:
                top = np.sort(sc, axis=1)
                bound = 1e-13 * np.max(np.abs(X) @ np.abs(W.T) + 1, axis=1)
                keep = (top[:, -1] - top[:, -2]) >= bound
            left_out = int(n - keep.sum())
            print(f"decide {storage} n={n} d={d} k={k}: left out {left_out}")
            assert left_out <= 0.01 * n, (n, d, k, left_out)
            assert np.array_equal(cls[keep], want[keep]), (n, d, k, np.flatnonzero(cls != want)[:5])
            assert np.array_equal(data.decide_multi(W), cls)
        # ties go to the lowest column: columns 2 and 3 repeat columns 1 and 0
        W = rng.standard_normal((3, d))
        sc = X @ W.T
        top = np.sort(sc, axis=1)
        keep = (top[:, -1] - top[:, -2]) >= 1e-13 * np.max(np.abs(X) @ np.abs(W.T) + 1, axis=1)
        cls = data.decide_multi(np.stack([W[0], W[1], W[1], W[0], W[2]]))
        assert np.array_equal(cls[keep], np.array([0, 1, 4], dtype=np.int32)[np.argmax(sc, axis=1)][keep]), (n, d)
        data.close()
    with pytest.raises(ValueError):
        S(8, 4, "erm", storage=storage, objective_only=True).decide_multi(np.zeros((2, 5)))


def _blobs(n, d, seed):
    rng = np.random.default_rng(seed)
    centres = 6.0 * rng.standard_normal((3, d)) / np.sqrt(d)      # drawn first: the same for every n
    labels = rng.integers(0, 3, size=n)
    X = rng.standard_normal((n, d)) + centres[labels]
    return X, np.array(["a", "b", "c"])[labels]


def test_one_vs_rest_end_to_end(R):
    """a separable 3-class problem: predict equals the arg-max over the scores of three standalone solvers built from
    (X, y_k).  Rank-weighted members of a group are bit-identical to standalone handles (test 1), so the weights agree
    exactly; rows whose two best scores are within 1e-13 (|x| . |w| + 1) of each other are left out of the comparison."""
    n, d, nit = 3000, 160, 40
    X, lab = _blobs(n, d, seed=2)
    Xt, labt = _blobs(800, d, seed=2)       # the same centres, other rows
    kw = dict(weight_function="superquantile", loss="binary_cross_entropy", l2_reg=0.01, args=[0.5])
    ovr = R.OneVsRest(X, lab, storage="f64", max_iter=nit, tol=0.0, **kw)
    assert list(ovr.classes_) == ["a", "b", "c"]
    W = _quiet(ovr.main_loop, verbose=False)
    assert W.shape == (d, 3)
    cnt = ovr.group.counters()
    assert cnt["shared_v"] == cnt["shared_q"] == nit * -(-3 // cnt["k_per_pass"])
    Wsa = []
    for c in ovr.classes_:
        s = R.ADMMmethod(X, np.where(lab == c, 1.0, -1.0), max_iter=nit, tol=0.0, storage="f64", **kw)
        Wsa.append(_quiet(s.main_loop, verbose=False).reshape(-1))
    Wsa = np.stack(Wsa, axis=1)
    assert np.array_equal(W, Wsa)
    pred = ovr.predict(Xt)
    sc = Xt @ Wsa
    top = np.sort(sc, axis=1)
    keep = (top[:, -1] - top[:, -2]) >= 1e-13 * np.max(np.abs(Xt) @ np.abs(Wsa) + 1, axis=1)
    assert keep.sum() >= 0.99 * len(keep)
    assert np.array_equal(pred[keep], ovr.classes_[np.argmax(sc, axis=1)][keep])
    acc = ovr.accuracy(Xt, labt)
    assert acc == np.mean(pred == labt) and acc > 0.95, acc
    # per-class test objectives with a list of test labels
    ovr2 = R.OneVsRest(X, lab, storage="f64", max_iter=5, tol=0.0, **kw)
    ovr2.group.start_store(Xt, [np.where(labt == c, 1.0, -1.0) for c in ovr2.classes_])
    _quiet(ovr2.main_loop, verbose=False)
    res = ovr2.group.final_res()
    assert len(res) == 3 and all(len(r[3]) == 6 and np.all(np.isfinite(r[3])) for r in res)
    assert len({r[3][-1] for r in res}) == 3          # three different label vectors: three different test losses
    ovr.close()
    ovr2.close()


def test_run_ovr_example():
    env = dict(os.environ, RBL_EXAMPLE_FAST="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "run_ovr.py")], capture_output=True, text=True,
                       timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = [ln for ln in r.stdout.splitlines() if ln.count(",") >= 5]
    assert len(rows) == 4, r.stdout
    acc = [float(ln.split(":")[1]) for ln in r.stdout.splitlines() if ln.startswith("multi-class test accuracy")]
    assert len(acc) == 1 and acc[0] > 0.8, r.stdout
