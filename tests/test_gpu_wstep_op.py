"""The operator w-step (csrc/wstep_op.hip): storage="csr" without the Gram matrix (RBL_CREATE_NO_GRAM, ``gram="none"``).

Kernel level, through rbl_k_wstep_op - the route a handle runs: the entries uploaded, both forms built, L from the power
iteration through the operator, then one w-step.  The ridge is held to the true residual ||A w - rho q|| formed on the host
from the CSR arrays, the lasso / elastic net to its KKT conditions; the same call repeated, and sized for another num_cu,
returns identical bits; the padding [d, ld) comes back +0.0.

Solver level: gram="none" against gram="dense" where both run, against tests/wstep_op_ref.py's ADMM (which never forms
D^T D) past the Gram route's width, a 200 000-column problem whose G would be 320 GB, groups and one-vs-rest members against
their standalone solves bit for bit, and the refusals of the C ABI.

C = 2048 is the chunk of the d-space reductions (wstep_op_plan.h)."""
import contextlib
import ctypes as C
import io

import numpy as np
import pytest

import wstep_op_ref as ref

pytestmark = pytest.mark.gpu
sp = pytest.importorskip("scipy.sparse")
ST = "csr"
CH = ref.CHUNK
KKT = 1e-9           # the bar of test_lasso_wstep_at_c5_width, relative to max(1, max|q|)
RES = 1e-9           # the project's bar for w-step optimality: ||A w - rho q|| <= RES ||rho q||
ITER = 1e-9          # the project's iterate bar
OBJ = 2.5e-7         # the project's whole-solve bar for the convex families (relative objective)


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


def _pad_is_plus_zero(w, d):
    return np.all(_bits(w[d:]) == 0)


def _close(a, b, bar):
    return float(np.max(np.abs(a - b))) <= bar * max(1.0, float(np.max(np.abs(b))))


# ---------------------------------------------------------------------------------------------------- kernel level
@pytest.fixture(scope="module")
def mats():
    """name -> (D, q): the small matrix, the first widths past the Gram route's cap (a column of ones last), and the
    widths around the reduction's chunk.  Built once, never modified."""
    out = {"small": ref.small_matrix()}
    for d in (16385, 20000):
        out[f"wide{d}"] = ref.wide_matrix(3000, d, per_row=6, seed=d, ones_column=True)
    for d in (CH - 1, CH, CH + 1, 2 * CH + 1):
        out[f"chunk{d}"] = ref.wide_matrix(500, d, per_row=6, seed=d, ones_column=True)
    res = {}
    for k, A in out.items():
        q = A.T @ np.random.default_rng(len(k)).standard_normal(A.shape[0])
        res[k] = (A, q)
    return res


ALL = ["small", "wide16385", "wide20000", f"chunk{CH - 1}", f"chunk{CH}", f"chunk{CH + 1}", f"chunk{2 * CH + 1}"]


@pytest.mark.parametrize("name", ALL)
@pytest.mark.parametrize("form", ["reg", "l2_free"])
def test_ridge_true_residual(R, mats, name, form):
    """CG on (rho D^T D + reg I) w = rho q, and with l2 per coordinate - the column of ones (the last one) free - at
    tol = 1e-12: the true residual, formed on the host in float64 from the CSR arrays, is at most 1e-9 ||rho q||"""
    A, q = mats[name]
    d = A.shape[1]
    rho = 0.37
    l2 = None
    if form == "l2_free":
        l2 = np.random.default_rng(d).uniform(0.1, 2.0, d)
        l2[d - 1] = 0.0
    w, it, status = R._lib.k_wstep_op(2, A, q, rho, reg=0.5, l2=l2, tol=1e-12)
    assert status == 1 and it > 0
    res = ref.ridge_residual(A, q, rho, 0.5, l2, w[:d])
    print(f"{name} {form}: {it} CG iterations, true residual {res:.3e}")
    assert res <= RES
    assert _pad_is_plus_zero(w, d)
    if name == "small":
        G = (A.T @ A).toarray()
        dense = np.linalg.solve(rho * G + (0.5 * np.eye(d) if l2 is None else np.diag(l2)), rho * q)
        assert _close(w[:d], dense, 1e-10)


@pytest.mark.parametrize("form", ["reg", "l1_free"])
def test_lasso_small_kkt(R, mats, form):
    """pure l1 on 300 x 37, scalar and per coordinate with the column of ones free.  n >> d: the problem is strongly convex
    and FISTA's step-size stop rule bounds the error"""
    A, q = mats["small"]
    d = A.shape[1]
    rho = 0.37
    qm = float(np.max(np.abs(q)))
    if form == "reg":
        reg, l1 = 2 * rho * 0.2 * qm, None
        w, it, status = R._lib.k_wstep_op(1, A, q, rho, reg=reg, tol=1e-13)
        kkt = ref.enet_kkt(A, q, rho, reg, None, w[:d])
    else:
        l1 = 2 * rho * 0.2 * qm * np.random.default_rng(1).uniform(0.5, 2.0, d)
        l1[d - 1] = 0.0
        w, it, status = R._lib.k_wstep_op(1, A, q, rho, l1=l1, tol=1e-13)
        kkt = ref.enet_kkt(A, q, rho, l1, None, w[:d])
        assert w[d - 1] != 0.0                       # the free coordinate is never thresholded
    print(f"small {form}: {it} FISTA iterations, KKT residual {kkt:.3e}, support {np.count_nonzero(w)}")
    assert status == 1 and 0 < np.count_nonzero(w[:d]) < d
    assert kkt <= KKT * max(1.0, qm)
    assert _pad_is_plus_zero(w, d)
    host, _, ok = ref.fista(A, q, rho, reg=(reg if l1 is None else 0.0), l1=l1, l2=None if l1 is None else 0.0, tol=1e-13)
    assert ok and _close(w[:d], host, 1e-9)


@pytest.mark.parametrize("name", [n for n in ALL if n != "small"])
def test_elastic_net_wide_kkt(R, mats, name):
    """Elastic net with every l2_j > 0 at the wide and the chunk-edge widths (the column of ones free of l1).  Pure l1 with
    n < d is not strongly convex: FISTA's stop rule - the step it took - would not certify a tight answer in bounded time
    there, so these shapes carry l2_j > 0, which makes the problem strongly convex whatever D is."""
    A, q = mats[name]
    d = A.shape[1]
    rho = 0.37
    qm = float(np.max(np.abs(q)))
    rng = np.random.default_rng(d + 1)
    l1 = 2 * rho * 0.3 * qm * rng.uniform(0.5, 2.0, d)
    l1[d - 1] = 0.0
    l2 = rho * rng.uniform(0.5, 2.0, d)
    w, it, status = R._lib.k_wstep_op(1, A, q, rho, l1=l1, l2=l2, tol=1e-13)
    kkt = ref.enet_kkt(A, q, rho, l1, l2, w[:d])
    print(f"{name}: {it} FISTA iterations, KKT residual {kkt:.3e}, support {np.count_nonzero(w)}")
    assert status == 1 and 0 < np.count_nonzero(w[:d]) < d
    assert kkt <= KKT * max(1.0, qm)
    assert _pad_is_plus_zero(w, d)


@pytest.mark.parametrize("name", ["small", f"chunk{2 * CH + 1}", "wide16385"])
def test_bits_do_not_depend_on_the_call_or_the_grid(R, mats, name):
    """the same call twice, and sized for num_cu = 1, 7 and the device's: identical bits, CG and FISTA"""
    A, q = mats[name]
    d = A.shape[1]
    rho = 0.37
    l1 = 2 * rho * 0.3 * float(np.max(np.abs(q))) * np.ones(d)
    l2 = rho * np.linspace(0.5, 2.0, d)
    for wstep, kw in ((2, dict(reg=0.5, tol=1e-12)), (2, dict(l2=l2, tol=1e-12)), (1, dict(l1=l1, l2=l2, tol=1e-11))):
        first = R._lib.k_wstep_op(wstep, A, q, rho, **kw)
        assert first[2] == 1
        for num_cu in (0, 1, 7):
            again = R._lib.k_wstep_op(wstep, A, q, rho, num_cu=num_cu, **kw)
            assert again[1:] == first[1:], (name, wstep, num_cu)
            assert np.array_equal(_bits(again[0]), _bits(first[0])), (name, wstep, num_cu)


def test_warm_start_and_iteration_cap(R, mats):
    A, q = mats["small"]
    d = A.shape[1]
    w, it, status = R._lib.k_wstep_op(2, A, q, 0.37, reg=0.5, tol=1e-12)
    w2, it2, status2 = R._lib.k_wstep_op(2, A, q, 0.37, reg=0.5, tol=1e-12, w0=w[:d])
    assert status2 == 1 and it2 <= 1 and _close(w2, w, 1e-12)        # started at the solution
    w3, it3, status3 = R._lib.k_wstep_op(2, A, q, 0.37, reg=0.5, tol=1e-12, max_inner=3)
    assert status3 == 0 and it3 >= 3                                 # the cap: whole batches, not converged


def test_kernel_entry_refusals(R, mats):
    A, q = mats["small"]
    L = R._lib
    with pytest.raises(ValueError, match="smoothed-l1.*diag\\(G\\)"):
        L.k_wstep_op(3, A, q, 0.37, reg=0.5)
    with pytest.raises(ValueError, match="wstep must be 1"):
        L.k_wstep_op(0, A, q, 0.37, reg=0.5)
    with pytest.raises(ValueError, match="penalties must be finite and >= 0"):
        L.k_wstep_op(2, A, q, 0.37, l2=-np.ones(A.shape[1]))
    n, d, ip, ix, va = L._csr_arrays(A)
    w = np.zeros(40)
    it, st = C.c_int(0), C.c_int(0)

    def call(n_, d_, ip_, q_, w_, rho=0.37, reg=0.5):
        return L.load().rbl_k_wstep_op(2, n_, d_, L.ptr(ip_), L.ptr(ix), L.ptr(va), L.ptr(q_), rho, reg, None, None, 1e-12,
                                       100, 0, L.ptr(w_), C.byref(it), C.byref(st))

    for args in ((n, 0, ip, q, w), (n, -3, ip, q, w), (0, d, ip, q, w), (n, d, None, q, w), (n, d, ip, None, w), (n, d, ip, q, None)):
        assert call(*args) == L.RBL_ERR_INVALID
        assert "bad argument" in L.last_error()
    assert call(n, d, ip, q, w, rho=0.0) == L.RBL_ERR_INVALID
    assert call(n, d, ip, q, w, reg=0.0) == L.RBL_ERR_INVALID
    assert call(n, d, ip, q, w) == L.RBL_OK


# ---------------------------------------------------------------------------------------------------- solver level
def _sparse_problem(n, d, density=0.15):
    from oracle import problems
    X, y = problems.make_problem(n, d, seed=900 + n + d)
    X = X * (np.random.default_rng(n + d).random(X.shape) < density)
    return sp.csr_matrix(X), y


def _run(R, A, y, nit, gram, **pr):
    m = R.ADMMmethod(A, y, max_iter=nit, tol=0.0, storage=ST, gram=gram, **pr)
    forms = [m._s.step(False).wstep_form for _ in range(nit)]
    return m, m._s.get_state(), forms


DENSE_CASES = {
    "erm_bce_l2": dict(weight_function="erm", loss="binary_cross_entropy", l2_reg=0.01),
    "superq_hinge_l2w_intercept": dict(weight_function="superquantile", loss="hinge", args=[0.5], fit_intercept=True,
                                       l2_weights=np.random.default_rng(61).uniform(0.005, 0.02, 61)),
    "erm_sqhinge_weighted": dict(weight_function="erm", loss="squared_hinge", l2_reg=0.01,
                                 sample_weight=0.5 + np.random.default_rng(400).random(400)),
}


@pytest.mark.parametrize("case", sorted(DENSE_CASES))
def test_no_gram_iterates_equal_the_gram_route(R, case):
    """400 x 61, 25 iterations: w, z and lambda of gram="none" agree with gram="dense" to 1e-9"""
    A, y = _sparse_problem(400, 61)
    pr = DENSE_CASES[case]
    nit = 25
    m0, dense, forms0 = _run(R, A, y, nit, "dense", **pr)
    m1, none, forms1 = _run(R, A, y, nit, "none", **pr)
    try:
        assert all(f == 4 for f in forms1), forms1
        assert all(f in (0, 1) for f in forms0), forms0
        assert m1.gram_info_["route"] == 0 and m0.gram_info_["route"] in (2, 3)
        assert m1.gram == "none" and m0.gram == "dense"
        with pytest.raises(ValueError, match='DTD: this solver runs with gram="none"'):
            m1.DTD
        assert m0.DTD.shape == (m0.num_feature, m0.num_feature)
        with pytest.raises(R._lib.RblError, match="no Gram matrix"):
            m1._s.buffer(R._lib.BUF_G)
        for key in ("w", "z", "lam"):
            diff = float(np.max(np.abs(none[key] - dense[key])))
            print(f"{case}: max |{key}(none) - {key}(dense)| = {diff:.3e} (max |{key}| = {np.max(np.abs(dense[key])):.3e})")
            assert _close(none[key], dense[key], ITER), (case, key, diff)
        assert none["rho"] == pytest.approx(dense["rho"], rel=1e-12)
    finally:
        m0._s.close()
        m1._s.close()


def test_no_gram_lasso_reaches_the_gram_route_objective(R):
    """erm / BCE / l1 on 400 x 61: FISTA on the operator against the exact active set of the Gram route - the objective
    after 25 iterations to 2.5e-7 relative; the largest iterate difference is printed, not asserted"""
    A, y = _sparse_problem(400, 61)
    pr = dict(weight_function="erm", loss="binary_cross_entropy", l1_reg=0.01)
    m0, dense, forms0 = _run(R, A, y, 25, "dense", **pr)
    m1, none, forms1 = _run(R, A, y, 25, "none", **pr)
    try:
        assert all(f == 4 for f in forms1), forms1
        assert 2 in forms0, forms0
        f0, f1 = m0._s.objective(dense["w"]), m1._s.objective(none["w"])
        print("objective dense / none:", f0, f1, "largest iterate difference:",
              {k: float(np.max(np.abs(none[k] - dense[k]))) for k in ("w", "z", "lam")})
        assert abs(f1 - f0) <= OBJ * max(1.0, abs(f0))
        assert m1.gram_info_["route"] == 0
    finally:
        m0._s.close()
        m1._s.close()


@pytest.fixture(scope="module")
def wide():
    """3000 x 20 000, six entries per row; the reference ADMM runs once per case and is shared"""
    X = ref.wide_matrix(3000, 20000, per_row=6, seed=77)
    y = np.where(np.random.default_rng(78).standard_normal(3000) > 0, 1.0, -1.0)
    D = sp.csr_matrix(sp.hstack([X, np.ones((3000, 1))]).multiply(-y[:, None]))
    return X, y, D


def test_wide_ridge_against_the_reference_admm(R, wide):
    """erm / BCE / l2 with an unpenalised intercept at d = 20 001: 10 iterations against wstep_op_ref.admm (exact w-steps
    through the n x n identity) to 1e-9; accuracy and objective on a sparse test matrix of the same width against NumPy"""
    X, y, D = wide
    d = D.shape[1]
    l2 = np.append(np.full(d - 1, 0.01), 0.0)
    want = ref.admm(D, "erm", "binary_cross_entropy", np.zeros(d), l2, 0.01, iters=10)
    m = R.ADMMmethod(X, y, "erm", "binary_cross_entropy", l2_reg=0.01, fit_intercept=True, storage=ST, max_iter=10, tol=0.0)
    try:
        assert m.gram == "none"                                       # "auto": ld = 20 004 > 16 384
        forms = [m._s.step(False).wstep_form for _ in range(10)]
        assert all(f == 4 for f in forms)
        got = m._s.get_state()
        for key in ("w", "z", "lam"):
            diff = float(np.max(np.abs(got[key] - want[key])))
            print(f"wide ridge: max |{key} - ref| = {diff:.3e} (max |{key}| = {np.max(np.abs(want[key])):.3e})")
            assert _close(got[key], want[key], ITER), (key, diff)
        # a sparse test matrix of the same width
        Xt = ref.wide_matrix(500, 20000, per_row=6, seed=79)
        yt = np.where(np.random.default_rng(80).standard_normal(500) > 0, 1.0, -1.0)
        coef = m.coef_
        from admm_for_rank_based_loss_amd.src.util.calculate_acc import calculate_accuracy
        acc = calculate_accuracy(coef, Xt, yt, storage=ST)
        assert acc == pytest.approx(float(np.mean(np.where(Xt @ coef >= 0, 1.0, -1.0) == yt)), abs=1e-12)
        obj = R.rankbasedObjective(Xt, yt, "erm", "binary_cross_entropy", l2_reg=0.01, storage=ST)
        from oracle import objective as oobj, weights
        f_np = oobj.objective_from_v("binary_cross_entropy", weights.get_weights("erm", 500)[0], -yt * (Xt @ coef), coef, 0.01, None)
        assert float(obj.get_arrogate_loss(coef.reshape(-1, 1))) == pytest.approx(f_np, rel=1e-10)
    finally:
        m._s.close()


def test_wide_elastic_net_against_the_reference_admm(R, wide):
    """aorr / hinge / elastic net with an unpenalised intercept at d = 20 001: the objective after 10 iterations against
    wstep_op_ref.admm to 2.5e-7 relative"""
    X, y, D = wide
    d = D.shape[1]
    rng = np.random.default_rng(81)
    l1w, l2w = rng.uniform(1e-5, 3e-5, d - 1), rng.uniform(0.005, 0.02, d - 1)
    pen = R._solver.resolve_penalty(d - 1, None, None, l1w, l2w, True)
    want = ref.admm(D, "aorr", "hinge", pen["l1"], pen["l2"], pen["reg"], args=[0.2, 0.8], iters=10)
    m = R.ADMMmethod(X, y, "aorr", "hinge", args=[0.2, 0.8], l1_weights=l1w, l2_weights=l2w, fit_intercept=True, storage=ST,
                     max_iter=10, tol=0.0)
    try:
        assert m.gram == "none"
        stats = [m._s.step(False) for _ in range(10)]
        assert all(st.wstep_form == 4 for st in stats)
        got = m._s.get_state()
        f = m._s.objective(got["w"])
        print("wide elastic net: objective", f, "reference", want["objective"], "inner iterations",
              [st.inner_iters for st in stats], "max |w - ref|", float(np.max(np.abs(got["w"] - want["w"]))))
        assert abs(f - want["objective"]) <= OBJ * max(1.0, abs(want["objective"]))
    finally:
        m._s.close()


def test_200000_columns_allocate_no_gram_matrix(R):
    """2000 x 200 000, six entries per row, gram="auto": the solver is created (G would be 320 GB), takes 5 iterations,
    and holds less than 1 GB of device memory"""
    import torch
    X = ref.wide_matrix(2000, 200000, per_row=6, seed=5)
    y = np.where(np.random.default_rng(6).standard_normal(2000) > 0, 1.0, -1.0)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    m = R.ADMMmethod(X, y, "erm", "binary_cross_entropy", l2_reg=0.01, storage=ST, max_iter=5, tol=0.0)
    try:
        used = free0 - torch.cuda.mem_get_info()[0]
        print(f"device memory in use after create: {used / 2**20:.1f} MiB")
        assert used < 2**30
        assert m.gram == "none" and m.gram_info_["route"] == 0
        stats = [m._s.step(True) for _ in range(5)]
        assert all(st.wstep_form == 4 and st.inner_iters > 0 for st in stats)
        assert all(np.isfinite([st.primal, st.dual, st.objective]).all() for st in stats)
        w = m._s.get_state()["w"]
        assert np.all(np.isfinite(w)) and np.any(w != 0.0)
        assert free0 - torch.cuda.mem_get_info()[0] < 2**30
    finally:
        m._s.close()


@contextlib.contextmanager
def _second_handle(R):
    """the rig of tests/test_gpu_csr_multi.py: the standalone solve runs beside a second live handle, as a group member does"""
    other = R.Solver(8, 4, "erm", reg=0.01, wstep=R._lib.WSTEP_L2, storage=ST)
    try:
        yield
    finally:
        other.close()


def _same_state(a, b, ctx):
    for key in ("w", "z", "lam"):
        assert np.array_equal(_bits(a[key]), _bits(b[key])), (ctx, key, float(np.max(np.abs(a[key] - b[key]))))
    assert a["rho"] == b["rho"], ctx


@pytest.mark.parametrize("share", [False, True])
def test_group_members_equal_their_standalone_solves(R, share):
    """three superquantile levels on 400 x 61 with gram="none": every member bit for bit its standalone gram="none" solve"""
    A, y = _sparse_problem(400, 61)
    nit = 8
    members = [dict(weight_function="superquantile", loss="binary_cross_entropy", l2_reg=0.01, args=[a]) for a in (0.5, 0.9, 0.3)]
    g = R.ADMMgroup(A, y, [dict(pr, gram="none", share_sparse=share) for pr in members], storage=ST, max_iter=nit, tol=0.0)
    try:
        _quiet(g.main_loop, False)
        assert g.gram_info_["route"] == 0
        assert all(st.wstep_form == 4 for st in g.last)
        cnt = g.counters()
        assert (cnt["shared_v"] > 0) == share, cnt
        states = [s._s.get_state() for s in g.solvers]
    finally:
        g.close()
    for k, pr in enumerate(members):
        with _second_handle(R):
            m, own, forms = _run(R, A, y, nit, "none", **pr)
            m._s.close()
        _same_state(states[k], own, (share, k))


@pytest.mark.parametrize("share", [False, True])
def test_one_vs_rest_members_equal_their_standalone_solves(R, share):
    A, _ = _sparse_problem(400, 61)
    labels = np.arange(400) % 3
    nit = 8
    ovr = R.OneVsRest(A, labels, l2_reg=0.01, storage=ST, max_iter=nit, tol=0.0, gram="none", share_sparse=share)
    try:
        _quiet(ovr.main_loop, False)
        assert ovr.gram_info_["route"] == 0
        assert all(st.wstep_form == 4 for st in ovr.group.last)
        states = [s._s.get_state() for s in ovr.group.solvers]
    finally:
        ovr.close()
    for k, c in enumerate(ovr.classes_):
        with _second_handle(R):
            m, own, forms = _run(R, A, np.where(labels == c, 1.0, -1.0), nit, "none", weight_function="erm",
                                 loss="binary_cross_entropy", l2_reg=0.01)
            m._s.close()
        _same_state(states[k], own, (share, k))


def test_mixed_gram_values_in_a_group_are_refused(R):
    A, y = _sparse_problem(400, 61)
    with pytest.raises(ValueError, match="problem 1: gram must be the same"):
        R.ADMMgroup(A, y, [dict(l2_reg=0.01, gram="none"), dict(l2_reg=0.02)], storage=ST)
    m = R.ADMMmethod(A, y, l2_reg=0.01, storage=ST, gram="none")
    try:
        with pytest.raises(ValueError, match="one data matrix, one route"):
            R.ADMMmethod(A, y, l2_reg=0.02, storage=ST, gram="dense", share_data=m)
    finally:
        m._s.close()


def _cfg(L, n, d, storage, wstep=2, objective_only=0):
    cfg = L.RblConfig()
    cfg.n, cfg.d, cfg.n_total, cfg.row_offset = n, d, n, 0
    cfg.loss, cfg.weight_function = L.LOSS["binary_cross_entropy"], L.WEIGHT["erm"]
    cfg.wstep, cfg.reg, cfg.smooth_t, cfg.tol, cfg.max_iter = wstep, 0.01, 1.0, 1e-4, 10
    cfg.storage, cfg.device, cfg.objective_only = L.STORAGE[storage], 0, objective_only
    return cfg


def test_create_time_refusals_of_the_c_abi(R):
    L = R._lib
    lib = L.load()
    h = C.c_void_p()
    # the Gram route past its width: refused at create, and the message names the way out
    assert lib.rbl_create(C.byref(_cfg(L, 50, 16385, "csr")), C.byref(h)) == L.RBL_ERR_INVALID and not h.value
    assert "RBL_CREATE_NO_GRAM" in L.last_error()
    assert lib.rbl_create_opts(C.byref(_cfg(L, 50, 16385, "csr")), 0, C.byref(h)) == L.RBL_ERR_INVALID
    # ... an objective-only handle of that width is what it was
    assert lib.rbl_create(C.byref(_cfg(L, 50, 16385, "csr", objective_only=1)), C.byref(h)) == L.RBL_OK
    lib.rbl_destroy(h)
    for storage in ("f32", "f64", "fp16"):
        assert lib.rbl_create_opts(C.byref(_cfg(L, 50, 20, storage)), L.CREATE_NO_GRAM, C.byref(h)) == L.RBL_ERR_INVALID
        assert "needs RBL_STORE_CSR" in L.last_error()
    assert lib.rbl_create_opts(C.byref(_cfg(L, 50, 20, "csr")), 2, C.byref(h)) == L.RBL_ERR_INVALID
    assert "unknown flag bits 0x2" in L.last_error()
    assert lib.rbl_create_opts(C.byref(_cfg(L, 50, 20, "csr")), 3, C.byref(h)) == L.RBL_ERR_INVALID
    assert lib.rbl_create_opts(C.byref(_cfg(L, 50, 20, "csr", wstep=L.WSTEP_SMOOTH_L1)), L.CREATE_NO_GRAM, C.byref(h)) == L.RBL_ERR_INVALID
    assert "diag(G)" in L.last_error()
    # a borrower of a no-Gram owner follows the same rules
    A, y = _sparse_problem(400, 61)
    m = R.ADMMmethod(A, y, l2_reg=0.01, storage=ST, gram="none")
    try:
        assert lib.rbl_create_shared(C.byref(_cfg(L, 400, 61, "csr", wstep=L.WSTEP_SMOOTH_L1)), m._s._h, C.byref(h)) == L.RBL_ERR_INVALID
        assert "diag(G)" in L.last_error() and not h.value
        assert lib.rbl_create_shared(C.byref(_cfg(L, 400, 61, "csr", wstep=L.WSTEP_L1)), m._s._h, C.byref(h)) == L.RBL_OK
        st = L.RblStats()
        assert lib.rbl_step(h, 0, C.byref(st)) == L.RBL_OK and st.wstep_form == 4
        lib.rbl_destroy(h)
    finally:
        m._s.close()
