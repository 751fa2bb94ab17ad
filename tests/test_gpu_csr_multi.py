"""Groups on storage="csr" with shared sparse passes (RBL_GROUP_SHARE_SPARSE, ``share_sparse=True``).

Kernel level (rbl_k_csr_gemv_multi / rbl_k_csr_gemvt_multi, the launchers of a group step with the caller's num_cu):
column j of a k-column launch has the bits of the single-column sparse pass on column j alone - for every k, every lane
group, every grid - a poisoned column leaves the others alone, dyadic inputs return an integer reference's bits, and
real-valued inputs stay within the project's bar of a longdouble product.  The entries check their own guard behind row n
(RBL_ERR_STATE if it was written), so a call that returns is a call that stayed inside its rows.

Solve level: a group with shared sparse passes reproduces the standalone storage="csr" solver and the unshared sparse group
bit for bit, with the counters of the dense group; OneVsRest and rbl_decide_multi's sparse route; dense storage ignores the
flag; the launchers' guards refuse data whose upload failed.

The v matrices have d = 512 columns, so at the lane group of 64 a row cannot be longer than 8 L = 512 entries: the row
"longer than 8 L" is there for L <= 32, the full row for every L."""
import contextlib
import io

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
sp = pytest.importorskip("scipy.sparse")
ST = "csr"
SEG = 2048                       # csc_plan.h: entries per segment of q = D^T c
KS = (1, 2, 3, 4)


@pytest.fixture(scope="module")
def R():
    import admm_for_rank_based_loss_amd as rbl
    if rbl._lib.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run the HIP library (no fallback)")
    return rbl


@pytest.fixture(scope="module")
def grids(R):
    """num_cu of the kernel-level calls: 1, 2 and the device's count"""
    s = R.Solver(8, 4, "erm", reg=0.01, wstep=R._lib.WSTEP_L2, storage=ST)
    cus = int(s.info()["num_cu"])
    s.close()
    assert cus > 2
    return (1, 2, cus)


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _csr(M, data):
    rows, cols = np.nonzero(M)                       # row-major: canonical
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=M.shape[0]))]).astype(np.int64)
    A = sp.csr_matrix((data, cols.astype(np.int32), indptr), shape=M.shape)
    assert A.has_canonical_format and A.nnz == rows.size
    return A


def _lanes_rule(nnz, n):
    """csr_lanes (spmv.hip): the narrowest group whose lanes take at most eight entries of an average row"""
    L = 4
    while L < 64 and 8 * L * n < nnz:
        L *= 2
    return L


# ------------------------------------------------------------------------------------------------ v = D w matrices
V_D = 512
V_CASES = [(L, per_row, n) for L, per_row in ((4, 3), (8, 40), (16, 100), (32, 200), (64, 400))
           for n in (64 * 256 // L - 1, 64 * 256 // L, 2 * (64 * 256 // L) + 37)]
assert (4, 3, 8229) in V_CASES and (64, 400, 549) in V_CASES


def _v_mask(L, per_row, n):
    rng = np.random.default_rng(1000 * L + n)
    M = rng.random((n, V_D)) < per_row / V_D
    M[0] = M[n // 2] = M[n - 1] = False              # empty rows: first, middle, last
    for r, c in ((1, 0), (n - 2, V_D - 1), (n // 3, 17)):
        M[r] = False
        M[r, c] = True                               # rows of one entry: first column, last column, one inside
    M[2] = True                                      # the full row
    if 8 * L < V_D:
        M[3] = False
        M[3, rng.choice(V_D, size=8 * L + 3, replace=False)] = True     # longer than 8 L, not full
    return M


_V = {}


def _v_case(R, L, per_row, n):
    """(A, W 4 x d, single-column results 4 x n) of a case, built and computed once"""
    key = (L, n)
    if key not in _V:
        M = _v_mask(L, per_row, n)
        rng = np.random.default_rng(7 * L + n)
        A = _csr(M, rng.standard_normal(int(M.sum())))
        rl = np.diff(A.indptr)
        assert (rl == 0).sum() >= 3 and (rl == 1).sum() >= 3 and rl.max() == V_D and _lanes_rule(A.nnz, n) == L
        assert 8 * L >= V_D or ((rl > 8 * L) & (rl < V_D)).any()
        W = rng.standard_normal((4, V_D))
        single = np.stack([R._lib.k_csr_gemv(A, W[j]) for j in range(4)])
        _V[key] = (A, W, single)
    return _V[key]


@pytest.mark.parametrize("L,per_row,n", V_CASES, ids=[f"L{L}-n{n}" for L, _, n in V_CASES])
def test_v_columns_have_the_single_column_bits(R, grids, L, per_row, n):
    A, W, single = _v_case(R, L, per_row, n)
    for k in KS:
        for num_cu in grids:
            V, lanes = R._lib.k_csr_gemv_multi(A, W[:k], num_cu)
            assert lanes == L, (lanes, L)
            assert V.shape == (k, n) and np.array_equal(_bits(V), _bits(single[:k])), (k, num_cu)
    empty = np.diff(A.indptr) == 0
    assert not _bits(single[:, empty]).any()                             # empty rows: +0.0
    # real-valued inputs against a longdouble product, the project's bar
    D = A.toarray()
    ref = (D.astype(np.longdouble) @ W.T.astype(np.longdouble)).T
    bar = 1e-13 * (np.abs(D) @ np.abs(W.T) + 1).T
    err = np.abs(single.astype(np.longdouble) - ref)
    print(f"v L={L} n={n}: max err/bar {float(np.max(err / bar)):.3f}")
    assert np.all(err <= bar)


@pytest.mark.parametrize("L,per_row,n", V_CASES[2::3], ids=[f"L{L}-n{n}" for L, _, n in V_CASES[2::3]])
def test_v_isolation_and_dyadic(R, L, per_row, n):
    A, W, single = _v_case(R, L, per_row, n)
    for k in (2, 3, 4):
        for t, poison in enumerate((np.nan, np.inf, -np.inf, 1e300)):
            j = t % k
            Wp = W[:k].copy()
            Wp[j] = poison
            V, _ = R._lib.k_csr_gemv_multi(A, Wp, 1)
            keep = [i for i in range(k) if i != j]
            assert np.array_equal(_bits(V[keep]), _bits(single[keep])), (k, j, poison)
            assert not np.isfinite(V[j][np.diff(A.indptr) > 0]).any() or poison == 1e300
    # dyadic: values in eighths (|x| <= 1), vectors in quarters (|w| <= 2): every product is a multiple of 1/32 and every
    # partial sum is below 512 * 2 - exact in 53 bits, whatever the order
    rng = np.random.default_rng(n)
    vi = rng.integers(-8, 9, size=A.nnz)
    wi = rng.integers(-8, 9, size=(4, V_D))
    Ad = sp.csr_matrix((vi / 8.0, A.indices, A.indptr), shape=A.shape)
    Ai = sp.csr_matrix((vi.astype(np.int64), A.indices, A.indptr), shape=A.shape)
    ref = np.stack([np.asarray(Ai @ wi[j].astype(np.int64)).reshape(-1) for j in range(4)]).astype(np.float64) / 32.0
    for k in KS:
        V, _ = R._lib.k_csr_gemv_multi(Ad, wi[:k] / 4.0, 1)
        assert np.array_equal(_bits(V), _bits(ref[:k])), k


# ---------------------------------------------------------------------------------------------- q = D^T c matrices
def _q_lengths():
    """40 000 x 7 (ld = 8: one padding column): columns of 0, 1, 2047, 2048, 2049 and 5000 entries and a column of ones over
    every row (20 segments: more than the 16 lanes that add a column's partial sums)"""
    n, d = 40000, 7
    rng = np.random.default_rng(77)
    M = np.zeros((n, d), dtype=bool)
    for j, length in enumerate((0, 1, 2047, 2048, 2049, 5000)):
        M[rng.choice(n, size=length, replace=False), j] = True
    M[:, 6] = True
    data = rng.standard_normal(int(M.sum()))
    A = _csr(M, data)
    A.data[A.indices == 6] = 1.0
    assert np.bincount(A.indices, minlength=d).tolist() == [0, 1, 2047, 2048, 2049, 5000, n]
    return A


def _q_many_columns():
    """300 x 600, every column non-empty: 600 segments, so with num_cu = 1 (64 blocks of 4 waves) a wave is in its third"""
    n, d = 300, 600
    rng = np.random.default_rng(78)
    M = rng.random((n, d)) < 0.05
    M[np.arange(d) % n, np.arange(d)] = True
    return _csr(M, rng.standard_normal(int(M.sum())))


_Q = {}


def _q_case(R, name):
    if name not in _Q:
        A = _q_lengths() if name == "lengths" else _q_many_columns()
        rng = np.random.default_rng(len(name))
        Cm = rng.standard_normal((4, A.shape[0]))
        single = np.stack([R._lib.k_csr_gemvt(A, Cm[j]) for j in range(4)])
        _Q[name] = (A, Cm, single)
    return _Q[name]


def _nseg_rule(A):
    """csc_plan_segptr: ceil(len / T) segments per non-empty column"""
    cl = np.bincount(A.indices, minlength=A.shape[1])
    return int(np.sum(-(-cl // SEG)))


@pytest.mark.parametrize("name", ["lengths", "many_columns"])
def test_q_columns_have_the_single_column_bits(R, grids, name):
    A, Cm, single = _q_case(R, name)
    n, d = A.shape
    ld = R._lib.storage_ld(d, ST)
    want_nseg = _nseg_rule(A)
    assert want_nseg == (28 if name == "lengths" else 600)
    for k in KS:
        for num_cu in grids:
            Q, nseg = R._lib.k_csr_gemvt_multi(A, Cm[:k], num_cu)
            assert nseg == want_nseg
            assert Q.shape == (k, ld) and np.array_equal(_bits(Q), _bits(single[:k])), (k, num_cu)
            assert not _bits(Q[:, d:]).any()                             # the padding [d, ld): +0.0 in every column
    cl = np.bincount(A.indices, minlength=d)
    assert not _bits(single[:, :d][:, cl == 0]).any()                    # empty columns: +0.0
    if name == "lengths":
        assert ld == d + 1 and (cl == 0).sum() == 1
    D = A.toarray()
    ref = (D.T.astype(np.longdouble) @ Cm.T.astype(np.longdouble)).T
    bar = 1e-13 * (np.abs(D.T) @ np.abs(Cm.T) + 1).T
    err = np.abs(single[:, :d].astype(np.longdouble) - ref)
    print(f"q {name}: max err/bar {float(np.max(err / bar)):.3f}")
    assert np.all(err <= bar)


@pytest.mark.parametrize("name", ["lengths", "many_columns"])
def test_q_isolation_and_dyadic(R, name):
    A, Cm, single = _q_case(R, name)
    n, d = A.shape
    for k in (2, 3, 4):
        for t, poison in enumerate((np.nan, np.inf, -np.inf, 1e300)):
            j = t % k
            Cp = Cm[:k].copy()
            Cp[j] = poison
            Q, _ = R._lib.k_csr_gemvt_multi(A, Cp, 1)
            keep = [i for i in range(k) if i != j]
            assert np.array_equal(_bits(Q[keep]), _bits(single[keep])), (k, j, poison)
            assert not _bits(Q[j, d:]).any()                             # no entries there: the padding stays +0.0
    # dyadic: values in eighths (|x| <= 1, the column of ones = 8/8), vectors in quarters (|c| <= 2): multiples of 1/32
    # with partial sums below 40 000 * 2 - exact in 53 bits
    rng = np.random.default_rng(n + d)
    vi = rng.integers(-8, 9, size=A.nnz)
    if name == "lengths":
        vi[A.indices == 6] = 8
    ci = rng.integers(-8, 9, size=(4, n))
    Ad = sp.csr_matrix((vi / 8.0, A.indices, A.indptr), shape=A.shape)
    Ai = sp.csr_matrix((vi.astype(np.int64), A.indices, A.indptr), shape=A.shape)
    ref = np.stack([np.asarray(Ai.T @ ci[j].astype(np.int64)).reshape(-1) for j in range(4)]).astype(np.float64) / 32.0
    for k in KS:
        Q, _ = R._lib.k_csr_gemvt_multi(Ad, ci[:k] / 4.0, 1)
        assert np.array_equal(_bits(Q[:, :d]), _bits(ref[:k])), k
        assert not _bits(Q[:, d:]).any()


def test_kernel_entries_check_their_arguments(R, grids):
    L = R._lib
    A, W, _ = _v_case(R, *V_CASES[0])
    for num_cu in (0, -1, grids[-1] + 1):
        with pytest.raises(ValueError, match="num_cu"):
            L.k_csr_gemv_multi(A, W[:2], num_cu)
        with pytest.raises(ValueError, match="num_cu"):
            L.k_csr_gemvt_multi(A, np.zeros((2, A.shape[0])), num_cu)
    with pytest.raises(ValueError, match="1..4 columns"):
        L.k_csr_gemv_multi(A, np.zeros((5, V_D)), 1)
    with pytest.raises(ValueError, match="1..4 columns"):
        L.k_csr_gemvt_multi(A, np.zeros((5, A.shape[0])), 1)


# ------------------------------------------------------------------------------------------------------ solve level
def _sparse_problem(n, d, intercept, density=0.15):
    """the sparse problem of tests/test_gpu_csr_storage.py"""
    from oracle import problems
    X, y = problems.make_problem(n, d, seed=700 + n + d, intercept=intercept)
    keep = np.random.default_rng(n + d).random(X.shape) < density
    if intercept:
        keep[:, -1] = True
    X = X * keep
    A = sp.csr_matrix(X)
    return A, A.toarray(), y


@contextlib.contextmanager
def _second_handle(R):
    """The l2 / smoothed w-step of a handle that is alone in its process on the device runs as one persistent launch; with
    a second live handle it runs the batched launches (wstep.hip: wp_plan - two persistent kernels side by side could wait
    for each other's CUs).  The two routes agree to rounding, not in bits.  A group always has several live handles, so
    the standalone solver it is compared with bit for bit runs beside a second (idle, tiny) handle as well: the same
    w-step route on both sides, as in test_relabelled_borrower_equals_a_handle_of_its_own."""
    other = R.Solver(8, 4, "erm", reg=0.01, wstep=R._lib.WSTEP_L2, storage=ST)
    try:
        yield
    finally:
        other.close()


def _standalone(R, A, y, pr, nit, tol, stop=None):
    """the member's own storage="csr" solve: (state where it stopped, steps it ran, redone z-steps, last residuals)"""
    with _second_handle(R):
        s = R.ADMMmethod(A, y, max_iter=nit, tol=tol, storage=ST, **pr)._s
        steps = redone = 0
        for _ in range(nit if stop is None else stop):
            st = s.step(False)
            steps += 1
            redone += int(st.zband == 2) + int(st.sort_passes == 12)
            if st.converged:
                break
        state = s.get_state()
        s.close()
    return state, steps, redone, (st.primal, st.dual)


def _group(R, A, y, members, tols, nit, share, storage=ST):
    """a group of ADMMmethod members stepped nit times: (states, counters, redone z-steps of live members)"""
    solvers = []
    for pr, tol in zip(members, tols):
        solvers.append(R.ADMMmethod(A, y, max_iter=nit, tol=tol, storage=storage, share_data=solvers[0] if solvers else None, **pr))
    g = R._solver.Group([s._s for s in solvers], share_sparse=share)
    live = [True] * len(solvers)
    redone, launches = 0, 0
    for _ in range(nit):
        if not any(live):
            break
        launches += -(-sum(live) // 4)
        stats = g.step(False)
        for k, st in enumerate(stats):
            if live[k]:
                redone += int(st.zband == 2) + int(st.sort_passes == 12)
                live[k] = not st.converged
    cnt = g.counters()
    states = [s._s.get_state() for s in solvers]
    g.close()
    for s in solvers:
        s._s.close()
    return states, cnt, redone, launches


def _same_state(a, b, ctx):
    for key in ("w", "z", "lam"):
        assert np.array_equal(_bits(a[key]), _bits(b[key])), (ctx, key, float(np.max(np.abs(a[key] - b[key]))))
    assert a["rho"] == b["rho"], ctx


def test_group_of_three_levels_shares_the_sparse_passes(R):
    A, X, y = _sparse_problem(1500, 80, False)
    nit, K = 6, 3
    members = [dict(weight_function="superquantile", loss="binary_cross_entropy", l2_reg=0.01, args=[a]) for a in (0.5, 0.9, 0.3)]
    shared, cnt, redone, launches = _group(R, A, y, members, [0.0] * K, nit, True)
    plain, cnt0, redone0, _ = _group(R, A, y, members, [0.0] * K, nit, False)
    assert cnt["k_per_pass"] == 4 and cnt["shared_v"] == cnt["shared_q"] == nit * -(-K // 4) == launches, cnt
    assert sum(cnt["single_passes"]) == K + redone, (cnt, redone)       # the first v = D w of every member, redone z-steps
    assert cnt0["k_per_pass"] == 1 and cnt0["shared_v"] == cnt0["shared_q"] == 0 and redone0 == redone, cnt0
    for k, pr in enumerate(members):
        own, steps, _, _ = _standalone(R, A, y, pr, nit, 0.0)
        assert steps == nit
        _same_state(shared[k], own, ("standalone", k))
        _same_state(shared[k], plain[k], ("unshared group", k))
        assert np.any(shared[k]["w"] != 0.0)


def test_group_pass_times(R):
    """rbl_group_profile / rbl_group_pass_times: events around the shared sparse passes, summed per step"""
    A, X, y = _sparse_problem(1500, 80, False)
    pr = dict(weight_function="erm", loss="binary_cross_entropy", l2_reg=0.01)
    solvers = []
    for k in range(5):
        solvers.append(R.ADMMmethod(A, y, max_iter=10, tol=0.0, storage=ST, share_data=solvers[0] if solvers else None, **pr))
    g = R._solver.Group([s._s for s in solvers], share_sparse=True)
    g.step(False)
    assert g.pass_times()["steps"] == 0                                  # not switched on: nothing recorded
    g.profile(True)
    for _ in range(3):
        g.step(False)
    pt = g.pass_times()
    assert pt["steps"] == 3 and pt["v"] > 0.0 and 0.0 < pt["pack"] < pt["q"], pt
    g.profile(False)
    g.step(False)
    assert g.pass_times()["steps"] == 0                                  # either call clears the sums
    state = [s._s.get_state() for s in solvers]
    g.close()
    plain, _, _, _ = _group(R, A, y, [pr] * 5, [0.0] * 5, 5, False)
    for k in range(5):
        _same_state(state[k], plain[k], k)                              # timing changes no iterate
    for s in solvers:
        s._s.close()


def test_mixed_group_of_six_with_members_that_converge(R):
    A, X, y = _sparse_problem(1500, 80, False)
    nit, K = 8, 6
    sw = 0.5 + np.random.default_rng(5).random(1500)
    members = [dict(weight_function="erm", loss="binary_cross_entropy", l1_reg=0.01),
               dict(weight_function="erm", loss="binary_cross_entropy", l2_reg=0.01),
               dict(weight_function="superquantile", loss="binary_cross_entropy", l2_reg=0.01, args=[0.5]),
               dict(weight_function="aorr", loss="hinge", l2_reg=1e-4, args=[0.2, 0.8]),
               dict(weight_function="extremile", loss="squared_hinge", l1_reg=0.01, args=[2.0]),
               dict(weight_function="erm", loss="binary_cross_entropy", l2_reg=0.05, sample_weight=sw)]
    # members 1 and 5 get the tol at which their own solve stops after its fourth / third step: a member converges when
    # both residuals are below tol (the residuals of a tol = 0 run, read off the standalone solver)
    tols = [0.0] * K
    for k, stop in ((1, 4), (5, 3)):
        tols[k] = float(np.nextafter(max(_standalone(R, A, y, members[k], nit, 0.0, stop=stop)[3]), np.inf))
    owns = [_standalone(R, A, y, pr, nit, tol) for pr, tol in zip(members, tols)]
    steps = [o[1] for o in owns]
    assert all(steps[k] == nit for k in (0, 2, 3, 4)) and steps[1] < nit and steps[5] < nit, steps
    want_launches = sum(-(-sum(1 for s in steps if s > i) // 4) for i in range(nit))
    assert want_launches < nit * 2                                       # the later batches shrink: 6 -> 4 live members
    shared, cnt, redone, launches = _group(R, A, y, members, tols, nit, True)
    plain, cnt0, _, _ = _group(R, A, y, members, tols, nit, False)
    assert cnt["k_per_pass"] == 4 and cnt["shared_v"] == cnt["shared_q"] == launches == want_launches, (cnt, want_launches)
    assert sum(cnt["single_passes"]) == K + redone, (cnt, redone)
    assert cnt0["k_per_pass"] == 1 and cnt0["shared_v"] == cnt0["shared_q"] == 0, cnt0
    for k in range(K):
        _same_state(shared[k], owns[k][0], ("standalone", k))             # a converged member: frozen at its own last iterate
        _same_state(shared[k], plain[k], ("unshared group", k))


def _blobs(n, d, seed, classes=3):
    rng = np.random.default_rng(seed)
    centres = 6.0 * rng.standard_normal((classes, d)) / np.sqrt(d)
    labels = rng.integers(0, classes, size=n)
    X = (rng.standard_normal((n, d)) + centres[labels]) * (rng.random((n, d)) < 0.3)
    return sp.csr_matrix(X), np.array(["a", "b", "c", "d", "e"])[labels]


@pytest.mark.parametrize("classes", [3, 5])
def test_one_vs_rest(R, classes):
    n, d, nit = 1500, 120, 10
    A, lab = _blobs(n, d, seed=2, classes=classes)
    At, _ = _blobs(600, d, seed=2, classes=classes)
    kw = dict(weight_function="superquantile", loss="binary_cross_entropy", l2_reg=0.01, args=[0.5])
    ovr = R.OneVsRest(A, lab, storage=ST, max_iter=nit, tol=0.0, share_sparse=True, **kw)
    W = _quiet(ovr.main_loop, verbose=False)
    cnt = ovr.group.counters()
    assert cnt["k_per_pass"] == 4 and cnt["shared_v"] == cnt["shared_q"] == nit * -(-classes // 4), cnt
    plain = R.OneVsRest(A, lab, storage=ST, max_iter=nit, tol=0.0, **kw)
    Wp = _quiet(plain.main_loop, verbose=False)
    cnt0 = plain.group.counters()
    assert cnt0["k_per_pass"] == 1 and cnt0["shared_v"] == cnt0["shared_q"] == 0, cnt0
    assert W.shape == (d, classes) and np.array_equal(_bits(W), _bits(Wp))
    pred, pred_p = ovr.predict(At), plain.predict(At)
    assert np.array_equal(pred, pred_p)
    # rbl_decide_multi's sparse route (one launch of 3 columns; 4 + 1 with five classes) against NumPy, on the rows whose
    # two best scores are further apart than the rounding of a score
    Xt = At.toarray()
    sc = Xt @ W
    top = np.sort(sc, axis=1)
    keep = (top[:, -1] - top[:, -2]) >= 1e-13 * np.max(np.abs(Xt) @ np.abs(W) + 1, axis=1)
    assert keep.sum() >= 0.99 * len(keep)
    assert np.array_equal(pred[keep], ovr.classes_[np.argmax(sc, axis=1)][keep])
    assert len(set(pred.tolist())) == classes
    ovr.close()
    plain.close()


def test_dense_storage_ignores_the_flag(R):
    A, X, y = _sparse_problem(1500, 80, False)
    nit = 5
    members = [dict(weight_function="superquantile", loss="binary_cross_entropy", l2_reg=0.01, args=[a]) for a in (0.5, 0.9, 0.3)]
    on, cnt_on, _, _ = _group(R, X, y, members, [0.0] * 3, nit, True, storage="f64")
    off, cnt_off, _, _ = _group(R, X, y, members, [0.0] * 3, nit, False, storage="f64")
    assert cnt_on == cnt_off and cnt_on["k_per_pass"] >= 2 and cnt_on["shared_v"] == cnt_on["shared_q"] == nit, (cnt_on, cnt_off)
    for k in range(3):
        _same_state(on[k], off[k], k)
    g = R.ADMMgroup(X, y, [dict(pr, share_sparse=True) for pr in members], storage="f64", max_iter=2, tol=0.0)
    _quiet(g.main_loop, verbose=False)
    assert g.counters()["k_per_pass"] == cnt_on["k_per_pass"]
    g.close()


def test_launcher_guards_after_a_failed_upload(R):
    """the owner's upload fails (a column index out of range: refused by the forming kernel, nothing faults) under two
    borrowers that have their v = D w; a group with the flag then meets the multi-column launcher's guard at its first
    step - RBL_ERR_STATE, nothing launched on entries that are not there - and works after a valid upload"""
    L = R._lib
    n, d = 3000, 8
    rng = np.random.default_rng(31)
    y = np.where(rng.random(n) < 0.5, 1.0, -1.0)
    one = sp.csr_matrix((rng.standard_normal(n), rng.integers(0, d, size=n).astype(np.int32), np.arange(n + 1, dtype=np.int64)), shape=(n, d))
    kw = dict(reg=0.01, wstep=L.WSTEP_L2, storage=ST, tol=0.0)
    owner = R.Solver(n, d, "erm", **kw)
    owner.set_data(one, y)
    owner.gram()
    bs = [R.Solver(n, d, "erm", share=owner, **kw) for _ in range(2)]
    for b in bs:
        b.step(False)
    bad = one.indices.copy()
    bad[5] = d
    code = owner.lib.rbl_set_data_csr(owner._h, L.ptr(one.indptr), L.ptr(bad), L.ptr(one.data), int(one.data.size),
                                      L.INDEX_DTYPE[one.indptr.dtype], L.SOURCE_DTYPE[one.data.dtype], L.MEM_HOST, L.ptr(y),
                                      L.SCALING["none"], 0)
    with pytest.raises(ValueError, match="is outside"):
        L.check(code)
    g = R._solver.Group(bs, share_sparse=True)
    with pytest.raises(L.RblError, match="csr gemvt multi: the data are not complete") as e:
        g.step(False)
    assert e.value.code == L.RBL_ERR_STATE
    owner.set_data(one, y)
    owner.gram()
    for _ in range(2):
        stats = g.step(True)
    assert all(np.isfinite(st.objective) and np.isfinite(st.primal) for st in stats)
    cnt = g.counters()
    assert cnt["k_per_pass"] == 4 and cnt["shared_q"] == 2 and cnt["shared_v"] == 2, cnt
    g.close()
    for s in bs + [owner]:
        s.close()
