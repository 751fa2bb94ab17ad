"""fp16 (IEEE binary16) storage of D on the device: include/rbl.h RBL_STORE_F16, ``storage="fp16"``.

The contract is the one fp32 storage has: the device solves, in fp64 arithmetic and with the same iterates, the problem
whose data matrix is the STORED one.  half -> double is exact, so every comparison below hands the oracle / NumPy side
``_lib.storage_round(X, "fp16")`` and uses the tolerances the f32 tests use for the same check (tests/test_gpu_widths.py,
test_gpu_kernels.py, test_gpu_group.py, test_gpu_labels.py, test_gpu_dist.py) - no new ones.

Packets per row with fp16 storage: ld / 8.  Rows of <= 32 packets (ld <= 256) take k_gemv / k_gemvt; 33 .. 512 packets
(ld <= 4096) the v-only / q-only single-sweep instances P = 1 / 2 / 4 / 8; the fused erm pass runs wave-per-row up to
P = 4 (ld <= 2048) and workgroup-per-row with 1 .. 4 packets per thread up to ld = 16384; the shared group passes cover
256 < ld <= 2048.
"""
import contextlib
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ST = "fp16"


@pytest.fixture(scope="module")
def R():
    import admm_for_rank_based_loss_amd as rbl
    if rbl._lib.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run the HIP library (no fallback)")
    return rbl


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------ 1. upload
@pytest.mark.parametrize("d", [1, 7, 8, 9, 333, 1000, 1001])
def test_upload_rounds_once_and_pads(R, d):
    L = R._lib
    rng = np.random.default_rng(d)
    n = 257
    X = rng.standard_normal((n, d)) * 10.0 ** rng.integers(-6, 4, size=(n, d))     # subnormal halves up to ~4e4
    X[0, 0] = 65504.0
    X[1, 0] = 1e-9                                                                 # underflows to 0: rounding, no error
    X[2, 0] = -(1.0 + 2.0 ** -11)                                                  # a tie: to even
    y = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    s = R.Solver(n, d, "erm", reg=0.01, storage=ST)
    assert s.info()["ld"] == L.storage_ld(d, ST) == (d + 7) // 8 * 8
    s.set_data(X, y)
    ref = -y[:, None] * L.storage_round(X, ST)
    got = s.get_D()
    assert np.array_equal(_bits(got + 0.0), _bits(ref + 0.0)), np.argwhere(got != ref)[:5]
    # the padded columns are zero: v = D w does not see what lies beyond d
    s.close()


def test_upload_rejects_what_does_not_fit(R):
    rng = np.random.default_rng(1)
    n, d = 300, 40
    X = rng.standard_normal((n, d))
    y = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    bad = X.copy()
    bad[3, 2] = 1e5
    bad[200, 39] = -7e4
    s = R.Solver(n, d, "erm", reg=0.01, storage=ST)
    with pytest.raises(ValueError, match=r"fp16 storage: 2 finite entries do not fit float16 .* first at row 3, column 2"):
        s.set_data(bad, y)
    with pytest.raises(Exception):          # the handle is left without data
        s.step(False)
    s.close()
    with pytest.raises(ValueError, match="fp16 storage: 2 finite entries do not fit float16"):
        R._lib.storage_round(bad, ST)       # the host-side check reads alike
    t = R.Solver(n, d, "erm", reg=0.01, storage=ST)
    t.set_data(X, y)                        # a fresh handle, valid data
    assert np.array_equal(t.get_D(), -y[:, None] * R._lib.storage_round(X, ST))
    tiny = np.full((n, d), 1e-9)
    t2 = R.Solver(n, d, "erm", reg=0.01, storage=ST)
    t2.set_data(tiny, y)
    assert np.all(t2.get_D() == 0.0)
    t.close()
    t2.close()
    # the f32 / f64 handles are as they were
    with pytest.raises(ValueError, match="storage must be one of"):
        R.Solver(n, d, "erm", reg=0.01, storage="f16")


# ----------------------------------------------------------------------------------------------------- 2. kernels
def test_gemv_gemvt(R):
    """tests/test_gpu_kernels.py::test_gemv_gemvt at one width per fp16 instance: lane groups of 1 .. 32 (ld <= 256), the
    wave-per-row range P = 1 / 2 / 4 / 8 (k_gemv; q takes SE_QONLY there), wide rows (LDS-staged k_gemv, k_gemvt with
    4 and 8 packets per thread), with and without row tails"""
    L = R._lib
    rng = np.random.default_rng(5)
    for n, d in [(1, 1), (17, 7), (64, 9), (257, 24), (300, 40), (1000, 100), (513, 200), (2000, 256), (2000, 300),
                 (63, 333), (1001, 1000), (700, 1001), (512, 2000), (300, 2500), (333, 4096), (150, 5000), (150, 9000)]:
        D = L.storage_round(rng.standard_normal((n, d)), ST)
        w, c = rng.standard_normal(d), rng.standard_normal(n)
        v, q = L.k_gemv(D, w, ST), L.k_gemvt(D, c, ST)
        assert np.max(np.abs(v - D @ w)) <= 1e-13 * np.max(np.abs(D) @ np.abs(w) + 1), (n, d)
        assert np.max(np.abs(q - D.T @ c)) <= 1e-13 * np.max(np.abs(D.T) @ np.abs(c) + 1), (n, d)


def test_multi_column_passes(R):
    """tests/test_gpu_group.py::test_multi_column_passes with fp16 storage: k in {1 .. 5} columns; widths below, inside
    (P = 1, 2, 4) and above the shared range"""
    L = R._lib
    rng = np.random.default_rng(11)
    for n, d in [(63, 130), (4099, 300), (63, 1000), (4099, 1000), (63, 1001), (700, 2048), (63, 2500)]:
        D = L.storage_round(rng.standard_normal((n, d)), ST)
        for k in (1, 2, 3, 4, 5):
            W, Cm = rng.standard_normal((k, d)), rng.standard_normal((k, n))
            V, Q = L.k_gemv_multi(D, W, ST), L.k_gemvt_multi(D, Cm, ST)
            bv = 1e-13 * np.max(np.abs(D) @ np.abs(W.T) + 1, axis=0)
            bq = 1e-13 * np.max(np.abs(D.T) @ np.abs(Cm.T) + 1, axis=0)
            ev = np.max(np.abs(V - (D @ W.T).T), axis=1)
            eq = np.max(np.abs(Q - (D.T @ Cm.T).T), axis=1)
            print(f"multi fp16 n={n} d={d} k={k}: max err V {ev.max():.2e} (bound {bv.min():.2e}) Q {eq.max():.2e} (bound {bq.min():.2e})")
            assert np.all(ev <= bv), (n, d, k, ev, bv)
            assert np.all(eq <= bq), (n, d, k, eq, bq)
            for j in {0, k - 1}:
                assert np.max(np.abs(V[j] - L.k_gemv(D, W[j], ST))) <= bv[j], (n, d, k, j)
                assert np.max(np.abs(Q[j] - L.k_gemvt(D, Cm[j], ST))) <= bq[j], (n, d, k, j)
            assert np.array_equal(L.k_gemv_multi(D, W, ST), V)          # bit-reproducible from run to run
            assert np.array_equal(L.k_gemvt_multi(D, Cm, ST), Q)


def test_gram(R):
    """G = D^T D by the fp64 MFMA on halves widened in registers (tests/test_gpu_kernels.py::test_gram_mfma and
    test_gpu_widths.py::test_gram_at_c5_width's bound); 300 and 4097 have tile tails; G is symmetric exactly"""
    L = R._lib
    rng = np.random.default_rng(7)
    for n, d in [(5, 3), (100, 17), (1000, 100), (3000, 129), (4001, 300), (900, 1000), (500, 4097)]:
        D = L.storage_round(rng.standard_normal((n, d)), ST)
        G = L.k_gram(D, ST)
        assert np.max(np.abs(G - D.T @ D)) <= 1e-12 * n, (n, d, np.max(np.abs(G - D.T @ D)))
        assert np.array_equal(G, G.T), (n, d)


# ------------------------------------------------------------------------- 3. iterates against the oracle's exact mode
FAM = {
    "superq": dict(weight_function="superquantile", loss="binary_cross_entropy", l2_reg=0.01, args=[0.5]),
    "aorr_hinge": dict(weight_function="aorr", loss="hinge", l2_reg=1e-4, args=[0.2, 0.8]),
    "ehrm": dict(weight_function="ehrm", loss="binary_cross_entropy", l2_reg=0.01, B=-5),
    "extremile_l1": dict(weight_function="extremile", loss="binary_cross_entropy", l1_reg=0.01, args=[2.0]),
}

# (family, rows, columns, intercept column) -> the SE_VONLY / SE_QONLY instance in the comment
WIDTHS = [
    ("superq", 3001, 300, False),        # P = 1
    ("extremile_l1", 3001, 333, False),  # P = 1, padded columns (d % 8 != 0), lasso w-step
    ("superq", 3008, 600, False),        # P = 2, whole super-batches only
    ("aorr_hinge", 3003, 520, False),    # P = 2
    ("superq", 3000, 1000, False),       # P = 4: C2sq's width
    ("aorr_hinge", 3000, 1000, True),    # C3's width: d = 1001 with the intercept column, ld = 1008
    ("ehrm", 2999, 1000, False),         # C4's width
    ("superq", 3001, 1500, False),       # P = 4
    ("ehrm", 1999, 2500, False),         # P = 8
    ("superq", 17, 2100, False),         # P = 8, one super-batch + 1 row
    ("superq", 1200, 4096, False),       # the widest supported row
]


def _run_gpu(R, X, y, kw, nit, no_fuse):
    if no_fuse:
        os.environ["RBL_NO_FUSE"] = "1"       # read by rbl_create
    try:
        s = R.ADMMmethod(X, y, max_iter=nit, tol=0.0, storage=ST, **kw)._s
    finally:
        os.environ.pop("RBL_NO_FUSE", None)
    hist, fv = [], 0
    for _ in range(nit):
        st = s.step(True)
        hist.append((st.primal, st.dual, st.rho, st.objective, st.ehrm_branch))
        fv += st.fused_v
    return np.array(hist), s.get_state(), fv


@pytest.mark.parametrize("fam,n,d,intercept", WIDTHS, ids=[f"{c[0]}-{c[1]}x{c[2] + (1 if c[3] else 0)}" for c in WIDTHS])
def test_rank_weighted_iterates(R, fam, n, d, intercept):
    """tests/test_gpu_widths.py::test_rank_weighted_iterates_at_bench_widths transposed to fp16 storage"""
    from oracle import problems, admm
    kw = FAM[fam]
    X, y = problems.make_problem(n, d, seed=1000 + d + n, intercept=intercept)
    X = R._lib.storage_round(X, ST)          # what the device stores: the oracle sees the same D
    nit = 8
    ref = admm.admm_solve(X, y, max_iter=nit, mode="exact", tol=0.0, **kw)
    tol = 1e-9 if kw["loss"] == "binary_cross_entropy" else 1e-7     # hinge: the kinks amplify rounding
    hf, sf, nfv = _run_gpu(R, X, y, kw, nit, no_fuse=False)
    hu, su, nuv = _run_gpu(R, X, y, kw, nit, no_fuse=True)
    assert nfv == nit and nuv == 0          # the v-only single-sweep kernel really ran / really did not
    for name, h, st in (("fused", hf, sf), ("unfused", hu, su)):
        assert np.allclose(h[:, 2], ref.rho, rtol=1e-15), name
        assert np.allclose(h[:, 0], ref.primal, rtol=tol, atol=tol), (name, h[:, 0], ref.primal)
        assert np.allclose(h[:, 1], ref.dual, rtol=tol, atol=tol), name
        assert np.allclose(h[:, 3], ref.objective[1:], rtol=tol, atol=tol), name
        if fam == "ehrm":
            assert [int(b) for b in h[:, 4]] == [0 if b == "a" else 1 for b in ref.branch], name
        assert np.max(np.abs(st["w"] - ref.w)) <= tol * max(1.0, np.max(np.abs(ref.w))), name
        assert np.max(np.abs(st["z"] - ref.z)) <= 10 * tol * max(1.0, np.max(np.abs(ref.z))), name
        assert np.max(np.abs(st["lam"] - ref.lam)) <= 10 * tol * max(1e-3, np.max(np.abs(ref.lam))), name
    # the two device paths differ only in the order of the fp64 sums of one row
    assert np.max(np.abs(sf["lam"] - su["lam"])) <= 1e-11 * max(1e-3, np.max(np.abs(su["lam"])))
    assert np.max(np.abs(sf["w"] - su["w"])) <= 1e-11 * max(1.0, np.max(np.abs(su["w"])))


# ------------------------------------------------------------------------------------------- 4. the erm single sweep
@pytest.mark.parametrize("rows,cols,loss,reg_kind", [
    (901, 333, "binary_cross_entropy", "l1_reg"),      # wave-per-row P = 1, padded columns
    (645, 1001, "hinge", "l2_reg"),                    # P = 2, d = 1001
    (5, 1100, "binary_cross_entropy", "l2_reg"),       # P = 4, fewer rows than one super-batch
    (1030, 1500, "binary_cross_entropy", "l2_reg"),    # P = 4, ragged last super-batch
    (300, 2048, "hinge", "l1_reg"),                    # the widest row of the wave-per-row kernel
    (700, 2500, "binary_cross_entropy", "l1_reg"),     # workgroup-per-row, 1 packet per thread
    (17, 2300, "hinge", "l2_reg"),                     # ... one full super-batch + 1 row
    (517, 5000, "hinge", "l2_reg"),                    # 2 packets per thread, ragged last super-batch
    (130, 9000, "binary_cross_entropy", "l2_reg"),     # 3 packets per thread
    (70, 15000, "hinge", "l1_reg"),                    # 4 packets per thread: the widest shape (w = 128 KB of LDS)
])
def test_single_sweep(rows, cols, loss, reg_kind):
    """tests/test_gpu_solver.py::test_single_sweep_wide_rows with fp16 storage: the fused pass against the two-sweep
    path on the same stored matrix"""
    here = os.path.dirname(os.path.abspath(__file__))
    runs = {}
    for name, env in (("fused", {}), ("unfused", {"RBL_NO_FUSE": "1"})):
        e = dict(os.environ)
        e.update(env)
        out = subprocess.run([sys.executable, os.path.join(here, "_fused_probe.py"), loss, reg_kind, str(rows), str(cols), ST],
                             env=e, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        runs[name] = json.loads(out.stdout.strip().splitlines()[-1])
    print(f"fused {runs['fused']['fused']} of 40, mispredicted {runs['fused']['mispredicted']}")
    assert runs["fused"]["fused"] >= 38 and runs["fused"]["mispredicted"] == 0
    assert runs["unfused"]["fused"] == 0
    hf, hu = np.array(runs["fused"]["hist"]), np.array(runs["unfused"]["hist"])
    assert np.array_equal(hf[:, 2], hu[:, 2])                       # same rho schedule
    assert np.allclose(hf[:, 0], hu[:, 0], rtol=1e-9, atol=1e-12)   # primal residual
    assert np.allclose(hf[:, 3], hu[:, 3], rtol=1e-10)              # objective
    for key in ("w", "z", "lam"):
        a, b = np.array(runs["fused"][key]), np.array(runs["unfused"][key])
        assert np.max(np.abs(a - b)) <= 1e-10 * max(1.0, np.max(np.abs(b))), key


def test_erm_iterates_vs_oracle_d1000(R):
    """25 erm iterations at C2's width against the oracle on the rounded matrix, asserted as
    tests/test_gpu_widths.py::test_iterates_at_c5_width_vs_oracle asserts its cases"""
    from oracle import problems, admm
    kw = dict(weight_function="erm", loss="binary_cross_entropy", l1_reg=0.01)
    X, y = problems.make_problem(3000, 1000, seed=4242)
    X = R._lib.storage_round(X, ST)
    nit = 25
    ref = admm.admm_solve(X, y, max_iter=nit, mode="exact", tol=0.0, **kw)
    s = R.ADMMmethod(X, y, max_iter=nit, tol=0.0, storage=ST, **kw)._s
    tol, fused = 1e-9, 0
    for i in range(nit):
        st = s.step(True)
        fused += st.fused
        assert abs(st.rho - ref.rho[i]) <= 1e-15 * ref.rho[i]
        assert abs(st.primal - ref.primal[i]) <= tol * max(1.0, ref.primal[i]), (i, st.primal, ref.primal[i])
        assert abs(st.dual - ref.dual[i]) <= tol * max(1.0, ref.dual[i]), i
        assert abs(st.objective - ref.objective[i + 1]) <= tol * max(1.0, abs(ref.objective[i + 1])), i
    assert fused == nit
    state = s.get_state()
    assert np.max(np.abs(state["w"] - ref.w)) <= tol * max(1.0, np.max(np.abs(ref.w)))
    assert np.max(np.abs(state["z"] - ref.z)) <= 10 * tol * max(1.0, np.max(np.abs(ref.z)))


# ------------------------------------------------------------------------------------------------ 5. groups, labels
def _redone(st):
    return int(st.zband == 2) + int(st.sort_passes == 12)


SQ = [dict(weight_function="superquantile", loss="binary_cross_entropy", l2_reg=0.01, args=[a]) for a in (0.5, 0.9, 0.3, 0.7, 0.2)]


def test_group_members_equal_standalone_handles(R):
    """five superquantile levels on one fp16 matrix at d = 1000 (tests/test_gpu_group.py::
    test_group_equals_standalone_and_passes_are_shared): every member bit-identical to a standalone fp16 handle, the
    passes shared four columns at a time, a member's own n x d launches only its first v = D w and redone z-steps"""
    from oracle import problems
    n, d, nit, K = 5000, 1000, 10, len(SQ)
    X, y = problems.make_problem(n, d, seed=100 + d)
    solvers = []
    for pr in SQ:
        solvers.append(R.ADMMmethod(X, y, max_iter=nit, tol=0.0, storage=ST, share_data=solvers[0] if solvers else None, **pr))
    g = R._solver.Group([s._s for s in solvers])
    redone, single = np.zeros((nit, K), dtype=int), []
    for i in range(nit):
        stats = g.step(want_objective=False)
        redone[i] = [_redone(st) for st in stats]
        single.append(np.array(g.counters()["single_passes"]))
    cnt = g.counters()
    single = np.array(single)
    states = [s._s.get_state() for s in solvers]
    g.close()
    assert cnt["k_per_pass"] == 4
    assert cnt["shared_v"] == cnt["shared_q"] == nit * -(-K // 4), cnt
    assert list(single[0]) == [1 + r for r in redone[0]], (single[0], redone[0])
    assert np.array_equal(single[-1] - single[0], redone[1:].sum(axis=0)), (single, redone)
    for k, pr in enumerate(SQ):       # (the group's handles stay alive: both sides run the same form of the w-step)
        s = R.ADMMmethod(X, y, max_iter=nit, tol=0.0, storage=ST, **pr)
        for _ in range(nit):
            s._s.step(False)
        alone = s._s.get_state()
        for key in ("w", "z", "lam"):
            assert np.array_equal(states[k][key], alone[key]), (k, key, np.max(np.abs(states[k][key] - alone[key])))
        assert states[k]["rho"] == alone["rho"]
        s._s.close()


def test_group_below_the_shared_widths_falls_back(R):
    """d = 200 (25 packets per row): each member runs its own passes and still matches its standalone handle (the bound
    tests/test_gpu_group.py uses for "same maths": 1e-11 relative) and the oracle on the rounded matrix"""
    from oracle import problems, admm
    n, d, nit = 3000, 200, 6
    X, y = problems.make_problem(n, d, seed=3)
    X = R._lib.storage_round(X, ST)
    members = SQ[:3]
    solvers = []
    for pr in members:
        solvers.append(R.ADMMmethod(X, y, max_iter=nit, tol=0.0, storage=ST, share_data=solvers[0] if solvers else None, **pr))
    g = R._solver.Group([s._s for s in solvers])
    for _ in range(nit):
        g.step(True)
    cnt = g.counters()
    assert cnt["k_per_pass"] == 1 and cnt["shared_v"] == 0 and cnt["shared_q"] == 0, cnt
    assert all(c >= 2 * nit for c in cnt["single_passes"]), cnt
    for pr, s in zip(members, solvers):
        mine = s._s.get_state()
        ref = admm.admm_solve(X, y, max_iter=nit, mode="exact", tol=0.0, **pr)
        assert np.max(np.abs(mine["w"] - ref.w)) <= 1e-9 * max(1.0, np.max(np.abs(ref.w)))
        a = R.ADMMmethod(X, y, max_iter=nit, tol=0.0, storage=ST, **pr)
        for _ in range(nit):
            a._s.step(False)
        alone = a._s.get_state()
        assert np.max(np.abs(mine["w"] - alone["w"])) <= 1e-11 * max(1.0, np.max(np.abs(alone["w"])))
        assert np.max(np.abs(mine["lam"] - alone["lam"])) <= 1e-11 * max(1e-3, np.max(np.abs(alone["lam"])))
        a._s.close()
    g.close()


def _blobs(n, d, seed):
    rng = np.random.default_rng(seed)
    centres = 6.0 * rng.standard_normal((3, d)) / np.sqrt(d)      # drawn first: the same for every n
    labels = rng.integers(0, 3, size=n)
    X = rng.standard_normal((n, d)) + centres[labels]
    return X, np.array(["a", "b", "c"])[labels]


def test_one_vs_rest(R):
    """tests/test_gpu_labels.py::test_one_vs_rest_end_to_end at fp16, d = 1000: the three relabelled members equal
    standalone fp16 solvers bit for bit, the passes are shared, predict is the NumPy arg-max on the ROUNDED test matrix"""
    n, d, nit = 3000, 1000, 12
    X, lab = _blobs(n, d, seed=2)
    Xt, labt = _blobs(800, d, seed=2)
    kw = dict(weight_function="superquantile", loss="binary_cross_entropy", l2_reg=0.01, args=[0.5])
    ovr = R.OneVsRest(X, lab, storage=ST, max_iter=nit, tol=0.0, **kw)
    W = _quiet(ovr.main_loop, verbose=False)
    assert W.shape == (d, 3)
    cnt = ovr.group.counters()
    assert cnt["k_per_pass"] == 4 and cnt["shared_v"] == cnt["shared_q"] == nit, cnt
    Wsa = []
    for c in ovr.classes_:
        s = R.ADMMmethod(X, np.where(lab == c, 1.0, -1.0), max_iter=nit, tol=0.0, storage=ST, **kw)
        Wsa.append(_quiet(s.main_loop, verbose=False).reshape(-1))
    Wsa = np.stack(Wsa, axis=1)
    assert np.array_equal(W, Wsa)
    pred = ovr.predict(Xt)
    Xr = R._lib.storage_round(Xt, ST)
    sc = Xr @ Wsa
    top = np.sort(sc, axis=1)
    keep = (top[:, -1] - top[:, -2]) >= 1e-13 * np.max(np.abs(Xr) @ np.abs(Wsa) + 1, axis=1)
    assert keep.sum() >= 0.99 * len(keep)
    assert np.array_equal(pred[keep], ovr.classes_[np.argmax(sc, axis=1)][keep])
    ovr.close()


# --------------------------------------------------------------------------------------------------- 6. generator
@pytest.mark.parametrize("n,d", [(5000, 300), (3000, 1001)])
def test_generator_rounds_once(R, n, d):
    """for one seed the fp16 matrix is the element-wise float16 rounding of the f64-storage generator's matrix - the
    statistics come from the unrounded draws and the standardised value is rounded once - under any row sharding"""
    import torch
    from admm_for_rank_based_loss_amd.dist import GpuEngine
    S = R._solver.Solver
    s64 = S(n, d, "erm", reg=0.01, storage="f64")
    s64.generate_synthetic(seed=7)
    want = s64.get_D().astype(np.float16).astype(np.float64)
    y64 = s64.labels()
    s64.close()
    s16 = S(n, d, "erm", reg=0.01, storage=ST)
    s16.generate_synthetic(seed=7)
    got = s16.get_D()
    assert np.array_equal(s16.labels(), y64)
    assert np.array_equal(got, want), (np.count_nonzero(got != want), np.max(np.abs(got - want)))
    s16.close()
    # two shards of the rows
    n0 = n // 2 + 1
    parts = [S(n0, d, "erm", reg=0.01, storage=ST, n_total=n, row_offset=0),
             S(n - n0, d, "erm", reg=0.01, storage=ST, n_total=n, row_offset=n0)]
    eng = [GpuEngine(p, 0) for p in parts]
    for p in parts:
        p.synth_local(seed=7)
    total = eng[0].buf("colstats") + eng[1].buf("colstats")
    for e in eng:
        e.buf("colstats").copy_(total)
    torch.cuda.synchronize()
    for p in parts:
        p.synth_finish()
    both = np.concatenate([p.get_D() for p in parts])
    assert np.array_equal(np.concatenate([p.labels() for p in parts]), y64)
    assert np.array_equal(both, want), (np.count_nonzero(both != want), np.max(np.abs(both - want)))
    for p in parts:
        p.close()


# ------------------------------------------------------------------------------------------------------ 7. memory
def test_fp16_handle_takes_little_more_than_half_the_memory(R):
    """device memory taken by creating + generating a 400 000 x 1000 erm handle: fp16 below 0.6 of f32.  With s bytes of
    per-row state the ratio is (2000 + s) / (4000 + s) < 0.6 for any s < 1000, and
    tests/test_gpu_group.py::test_borrowers_cost_little_device_memory holds per-row state below a quarter of an f32 row"""
    import torch
    S = R._solver.Solver
    n, d = 400_000, 1000

    def used():
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info(0)
        return total - free

    took = {}
    for storage in ("f32", ST):
        u0 = used()
        s = S(n, d, "erm", reg=0.01, wstep=R._lib.WSTEP_L1, storage=storage)
        s.generate_synthetic(seed=5)
        took[storage] = used() - u0
        s.close()
    print(f"400000 x 1000 erm handle: f32 {took['f32'] / 1e6:.1f} MB, fp16 {took[ST] / 1e6:.1f} MB, ratio {took[ST] / took['f32']:.3f}")
    assert took[ST] < 0.6 * took["f32"], took


# ----------------------------------------------------------------------------------------------- 8. row-sharded
def test_two_ranks_as_threads_match_single_handle(R, monkeypatch):
    """the threads-as-ranks rig of tests/test_gpu_dist.py (imported as it is), world 2, superquantile at fp16, against the
    single fp16 handle on the same generated data; bounds of test_eight_ranks_as_threads_match_single_handle"""
    import threading
    import torch  # noqa: F401
    from admm_for_rank_based_loss_amd import dist as _d  # noqa: F401
    from test_gpu_dist import _Hub, _thread_rank
    cfg = dict(n=50003, d=300, wf="superquantile", args=[0.5], loss="binary_cross_entropy", reg=0.01, wstep=2, iters=6, storage=ST)
    monkeypatch.setenv("RBL_NO_ZBAND", "1")          # the sort-based z-step on both sides, as in that test
    one = R.Solver(cfg["n"], cfg["d"], cfg["wf"], cfg["loss"], reg=cfg["reg"], wstep=cfg["wstep"], args=cfg["args"], tol=0.0, storage=ST)
    one.generate_synthetic(seed=12)
    one.gram()
    hist1 = []
    for _ in range(cfg["iters"]):
        st = one.step(True)
        hist1.append((st.primal, st.dual, st.rho, st.objective))
    s1 = one.get_state()
    one.close()
    world = 2
    hub, out, errs = _Hub(world), [None] * world, []
    ts = [threading.Thread(target=_thread_rank, args=(r, world, cfg, hub, out, errs)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(600)
    assert not errs, errs
    assert np.array_equal(out[0]["w"], out[1]["w"]) and np.array_equal(out[0]["hist"], out[1]["hist"])
    z2 = np.concatenate([r["z"] for r in out])
    assert np.max(np.abs(out[0]["w"] - s1["w"])) <= 1e-9 * max(1.0, np.max(np.abs(s1["w"])))
    assert np.max(np.abs(z2 - s1["z"])) <= 1e-8 * max(1.0, np.max(np.abs(s1["z"])))
    assert np.allclose(out[0]["hist"], np.array(hist1), rtol=1e-8, atol=1e-12)
