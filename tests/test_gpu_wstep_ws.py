"""The working-set lasso (csrc/wstep_ws.hip): l1_solver="working_set" - RBL_CREATE_WORKING_SET on a gram="none" handle.

Kernel level: the sub-Gram matrix from the entries (rbl_k_wset_gram) against A[:, S]^T A[:, S] to the fma chain's own bound,
symmetric in bits, the same bits for any insertion order and grid; the scan's choice (rbl_k_wset_scan) against the NumPy
rule of tests/wstep_ws_ref.py; whole w-steps (rbl_k_wstep_ws) held to the lasso KKT conditions on ALL columns - pure l1
with n < d included, which no other w-step of the library certifies -, to the independent solver's support, and to the
Gram route's exact kernel where both run.

Solver level: ten ADMM iterations at d = 20 001 against tests/wstep_op_ref.py's ADMM, groups and one-vs-rest members against
their standalone solves bit for bit, a second upload, a state set from outside, the default against the parent commit's
iterates (tests/golden/wstep_ws_parent_fista.npz: written by the parent commit's library on an MI355X), and the refusals of
the C ABI."""
import contextlib
import ctypes as C
import io
import os

import numpy as np
import pytest

import wstep_op_ref as opref
import wstep_ws_ref as ref

pytestmark = pytest.mark.gpu
sp = pytest.importorskip("scipy.sparse")
ST = "csr"
RHO = ref.RHO
KKT = 1e-9           # relative to max(1, max|q|), as in tests/test_gpu_wstep_op.py
ITER = 1e-9
OBJ = 2.5e-7
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wstep_ws_parent_fista.npz")


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


def _dev(ptr, cnt):
    import torch
    from admm_for_rank_based_loss_amd.dist import _DevArray
    torch.cuda.synchronize()
    return torch.as_tensor(_DevArray(ptr, cnt), device="cuda:0").cpu().numpy().copy()


def _plus_zero(a):
    return bool(np.all(_bits(a) == 0))


# ---------------------------------------------------------------------------------------------------- rbl_k_wset_gram
@pytest.fixture(scope="module")
def gmat():
    """300 x 150: about 8 % dense, column 11 empty, column 12 with one entry, row 5 with 100 entries (more than a wave),
    the last column all ones (300 entries: the wave loops over the column too)"""
    A = sp.random(300, 150, density=0.08, random_state=np.random.RandomState(4), format="lil", dtype=np.float64)
    A[:, 11] = 0.0
    A[:, 12] = 0.0
    A[40, 12] = -1.75
    A[5, :100] = np.random.default_rng(5).standard_normal(100)
    A[5, 11] = 0.0
    A[5, 12] = 0.0
    A[:, 149] = 1.0
    A = sp.csr_matrix(A)
    A.eliminate_zeros()
    A.sort_indices()
    assert A[:, 11].nnz == 0 and A[:, 12].nnz == 1 and A[5].nnz >= 98 and A[:, 149].nnz == 300
    return A


def _check_gram(R, A, cols, **kw):
    Gs = R._lib.k_wset_gram(A, cols, **kw)
    k = len(cols)
    As = sp.csc_matrix(A)[:, cols]
    want = (As.T @ As).toarray()
    absum = (abs(As).T @ abs(As)).toarray()
    m = np.diff(As.indptr).astype(np.float64)
    bound = (m[:, None] + 1.0) * 2.0 ** -53 * absum          # the fma chain's own bound, m the column's entry count
    err = np.abs(Gs[:k, :k] - want)
    assert np.all(err <= bound), float(np.max(err - bound))
    assert np.array_equal(_bits(Gs), _bits(Gs.T))            # symmetric in bits
    rest = np.ones((R._lib.WS_CAP, R._lib.WS_CAP), dtype=bool)
    rest[:k, :k] = False
    assert _plus_zero(Gs[rest])                              # unused slots: exactly zero
    return Gs


def test_gram_rows_against_the_float64_product(R, gmat):
    d = gmat.shape[1]
    cols = [149, 3, 11, 12, 77, 5, 0, 60, 148, 99]           # ones, empty, one entry, the columns of the long row
    Gs = _check_gram(R, gmat, cols)
    assert _plus_zero(Gs[2, :]) and Gs[3, 3] == 1.75 ** 2 and Gs[0, 0] == 300.0
    _check_gram(R, gmat, [d - 1])                            # S = {d - 1}
    _check_gram(R, gmat, [11])                               # |S| = 1, an empty column
    _check_gram(R, gmat, [])
    _check_gram(R, gmat, list(range(d)))                     # every column: the long row adds into 98 slots at once


def test_gram_bits_do_not_depend_on_order_calls_or_grid(R, gmat):
    cols = [149, 3, 11, 12, 77, 5, 0, 60, 148, 99, 20, 21, 22]
    k = len(cols)
    first = R._lib.k_wset_gram(gmat, cols)
    perm = np.random.default_rng(6).permutation(k)
    other = R._lib.k_wset_gram(gmat, [cols[i] for i in perm])
    assert np.array_equal(_bits(other[:k, :k]), _bits(first[np.ix_(perm, perm)]))
    # num_cu caps the grid at one block of four waves per unit: with num_cu = 1 a wave walks up to four of the 13 columns
    for kw in (dict(split=[3, 1, k - 4]), dict(split=[1] * k), dict(num_cu=1), dict(num_cu=2), dict(num_cu=1, split=[5, k - 5])):
        again = R._lib.k_wset_gram(gmat, cols, **kw)
        assert np.array_equal(_bits(again), _bits(first)), kw


def test_gram_at_full_capacity(R):
    """|S| = WS_CAP on 500 x 2049: sixteen launches of 64 columns, every slot in use"""
    A, _ = ref.fixture(500, 2049)
    cols = np.random.default_rng(8).permutation(2049)[:R._lib.WS_CAP]
    cols[0] = 2048                                           # the column of ones
    cols = list(dict.fromkeys(int(c) for c in cols))
    cols += [c for c in range(2049) if c not in set(cols)][:R._lib.WS_CAP - len(cols)]
    assert len(cols) == R._lib.WS_CAP
    Gs = _check_gram(R, A, cols)
    assert Gs[0, 0] == 500.0
    with pytest.raises(ValueError, match="appears twice"):
        R._lib.k_wset_gram(A, [1, 2, 1])
    with pytest.raises(ValueError, match="outside"):
        R._lib.k_wset_gram(A, [2049])


# ---------------------------------------------------------------------------------------------------- rbl_k_wset_scan
def _prescribed(d, ld, seed):
    rng = np.random.default_rng(seed)
    g = np.zeros(ld)
    g[:d] = np.round(rng.standard_normal(d) * 4.0) / 4.0     # quarter steps: many exact ties within and across chunks
    kappa = np.full(ld, 0.75)
    member = np.zeros(ld, dtype=np.int32)
    member[:d] = rng.random(d) < 0.05
    q = np.zeros(ld)
    q[:d] = rng.standard_normal(d)
    g[d - 1], member[d - 1] = -9.0, 0                        # a candidate in the last column
    g[7], g[1024], member[7], member[1024] = 5.0, -5.0, 0, 0   # a tie inside chunk 0
    kappa[3], g[3], member[3] = 0.0, 4.0, 0                  # a free coordinate
    return g, kappa, member, q


@pytest.mark.parametrize("d", [2047, 2048, 2049, 4097])
def test_scan_selects_what_the_numpy_rule_selects(R, d):
    L = R._lib
    ld = L.storage_ld(d, ST)
    g, kappa, member, q = _prescribed(d, ld, d)
    g[d:] = 100.0                                            # the padding is never chosen, whatever stands there
    for take in (L.WS_SELECT, 1):
        got = L.k_wset_scan(g, kappa, member, d=d, q=q, tol=1e-13, take=take)
        assert got == ref.select(g, kappa, member, d, q, 1e-13, take), (d, take)
    assert got[0] == d - 1
    # ties across chunks: the same violation in two chunks comes out in column order
    g2 = np.zeros(ld)
    g2[[5, d - 2]] = 2.0
    k2, m2 = np.full(ld, 0.5), np.zeros(ld, dtype=np.int32)
    assert L.k_wset_scan(g2, k2, m2, d=d) == ref.select(g2, k2, m2, d) == ([5, d - 2] if (d - 2) // ref.CHUNK > 0 else [5])
    # none: below the threshold everywhere; a threshold max|q| raises; every column a member
    assert L.k_wset_scan(np.full(ld, 0.5), k2, m2, d=d) == []
    assert L.k_wset_scan(g2, k2, m2, d=d, q=np.full(ld, 1e3), tol=1e-2) == []
    assert L.k_wset_scan(g, kappa, np.ones(ld, dtype=np.int32), d=d, q=q) == []


def test_scan_with_more_than_64_violating_chunks(R):
    """70 chunks, each with a candidate: the 64 largest, largest first, ties to the smaller column"""
    L = R._lib
    d = 70 * ref.CHUNK - 3
    ld = L.storage_ld(d, ST)
    g, kappa, member, q = _prescribed(d, ld, 70)
    want = ref.select(g, kappa, member, d, q, 1e-13)
    got = L.k_wset_scan(g, kappa, member, d=d, q=q, tol=1e-13)
    assert len(want) == 64 and got == want
    assert len({j // ref.CHUNK for j in got}) == 64


# ---------------------------------------------------------------------------------------------------- rbl_k_wstep_ws
@pytest.fixture(scope="module")
def fx():
    """(n, d) -> (D, q, max|q|, reg at kappa = 0.05 max|q|, the independent solver's w): tests/test_wstep_ws_host.py
    checks these on the CPU.  Built once, never modified."""
    out = {}
    for n, d in ref.SHAPES:
        A, q = ref.fixture(n, d)
        qm = float(np.max(np.abs(q)))
        reg = 2 * RHO * ref.KAPPA_FRAC * qm
        out[(n, d)] = (A, q, qm, reg, ref.independent_lasso(A, q, RHO, reg=reg))
    return out


@pytest.mark.parametrize("shape", ref.SHAPES)
def test_pure_l1_wide_meets_the_kkt_conditions(R, fx, shape):
    """pure lasso with n < d - not strongly convex, FISTA's stop rule certifies nothing there: the working set ends at a
    point that satisfies the KKT conditions on all d columns, with the independent solver's support"""
    A, q, qm, reg, w_ind = fx[shape]
    d = A.shape[1]
    W, reps = R._lib.k_wstep_ws(A, q, RHO, reg=reg, tol=1e-13)
    w, rep = W[0], reps[0]
    kkt = opref.enet_kkt(A, q, RHO, reg, None, w[:d])
    print(f"{shape}: KKT residual {kkt:.3e} (bar {KKT * max(1.0, qm):.3e}), support {rep['support']}, {rep}")
    assert kkt <= KKT * max(1.0, qm)
    assert rep["form"] == 5 and rep["left_route"] == 0
    assert _plus_zero(w[d:]) and _plus_zero(w[:d][w[:d] == 0])   # outside the support: +0.0 in bits, padding included
    assert np.array_equal(w[:d] != 0, w_ind != 0) and rep["support"] == np.count_nonzero(w_ind)
    assert np.max(np.abs(w[:d] - w_ind)) <= ITER * max(1.0, float(np.max(np.abs(w_ind))))
    assert rep["pass_pairs"] == rep["rounds"] - 1            # w = 0 in the first round: g = -q without a pass
    assert rep["slots"] == rep["rows_last"] == rep["rows_total"] and rep["evictions"] == 0


@pytest.mark.parametrize("shape", [(500, 2049), (3000, 16385)])
@pytest.mark.parametrize("form", ["scalar_l2", "per_coordinate"])
def test_elastic_net_meets_the_kkt_conditions(R, fx, shape, form):
    A, q, qm, reg, _ = fx[shape]
    d = A.shape[1]
    rng = np.random.default_rng(d + 1)
    if form == "scalar_l2":
        l1, l2 = np.full(d, reg), np.full(d, 0.5 * RHO)
    else:
        l1 = reg * rng.uniform(0.5, 2.0, d)
        l1[d - 1] = 0.0                                      # the column of ones is free
        l2 = RHO * rng.uniform(0.0, 1.0, d)
    W, reps = R._lib.k_wstep_ws(A, q, RHO, l1=l1, l2=l2, tol=1e-13)
    w, rep = W[0], reps[0]
    kkt = opref.enet_kkt(A, q, RHO, l1, l2, w[:d])
    print(f"{shape} {form}: KKT residual {kkt:.3e}, {rep}")
    assert kkt <= KKT * max(1.0, qm) and rep["form"] == 5 and _plus_zero(w[d:])
    if form == "per_coordinate":
        assert w[d - 1] != 0.0


def test_small_strongly_convex_problem_agrees_with_the_gram_route(R):
    """300 x 37: two exact solvers of a problem with a unique minimiser"""
    A = opref.small_matrix()
    q = A.T @ np.random.default_rng(5).standard_normal(A.shape[0])
    d = A.shape[1]
    qm = float(np.max(np.abs(q)))
    l1 = 2 * RHO * 0.2 * qm * np.random.default_rng(1).uniform(0.5, 2.0, d)
    l1[d - 1] = 0.0
    l2 = RHO * np.linspace(0.0, 1.0, d)
    G = (A.T @ A).toarray()
    want, _, form = R._lib.k_wstep_pen(G, q, RHO, l1=l1, l2=l2, tol=1e-13)
    W, reps = R._lib.k_wstep_ws(A, q, RHO, l1=l1, l2=l2, tol=1e-13)
    assert form == 2 and reps[0]["form"] == 5 and 0 < reps[0]["support"] < d
    assert np.max(np.abs(W[0][:d] - want)) <= ITER * max(1.0, float(np.max(np.abs(want))))
    assert _plus_zero(W[0][d:])
    for reg in (2 * RHO * 0.2 * qm,):                        # the scalar instance
        want, _ = R._lib.k_wstep(1, G, q, RHO, reg, tol=1e-13)
        W, reps = R._lib.k_wstep_ws(A, q, RHO, reg=reg, tol=1e-13)
        assert np.max(np.abs(W[0][:d] - want)) <= ITER * max(1.0, float(np.max(np.abs(want))))


def test_overflow_of_the_active_set_kernel_falls_to_fista_on_gs(R):
    """500 x 4097, kappa = 0.03 max|q|, l2_j in rho [0.5, 2]: more than 96 active coordinates - the restricted solve falls
    to FISTA on the sub-Gram matrix, the w-step stays on the route and meets the KKT conditions"""
    n, d, frac = ref.OVERFLOW
    A, q = ref.fixture(n, d)
    qm = float(np.max(np.abs(q)))
    l1, l2 = np.full(d, 2 * RHO * frac * qm), ref.overflow_l2(d)
    W, reps = R._lib.k_wstep_ws(A, q, RHO, l1=l1, l2=l2, tol=1e-13)
    w, rep = W[0], reps[0]
    kkt = opref.enet_kkt(A, q, RHO, l1, l2, w[:d])
    print(f"overflow: KKT residual {kkt:.3e}, {rep}")
    assert rep["fista_on_gs"] == 1 and rep["left_route"] == 0 and rep["form"] == 5
    assert rep["support"] > ref.FS_MAX
    assert kkt <= KKT * max(1.0, qm) and _plus_zero(w[d:])


def test_capacity_exhausted_leaves_the_route(R):
    """16 slots for a support of more than 100: the w-step leaves the route, reports form 4, and the operator FISTA still
    meets the KKT conditions (l2 > 0: strongly convex)"""
    n, d, frac = ref.OVERFLOW
    A, q = ref.fixture(n, d)
    qm = float(np.max(np.abs(q)))
    l1, l2 = np.full(d, 2 * RHO * frac * qm), ref.overflow_l2(d)
    W, reps = R._lib.k_wstep_ws(A, q, RHO, l1=l1, l2=l2, tol=1e-13, ws_cap=16)
    w, rep = W[0], reps[0]
    kkt = opref.enet_kkt(A, q, RHO, l1, l2, w[:d])
    print(f"capacity: KKT residual {kkt:.3e}, {rep}")
    assert rep["left_route"] == 1 and rep["form"] == 4 and rep["slots"] <= 16 and rep["support"] == -1
    assert kkt <= KKT * max(1.0, qm) and _plus_zero(w[d:])


def test_more_free_coordinates_than_slots_leaves_the_route(R):
    """20 unpenalised columns for 16 slots: S cannot hold what it must - the operator FISTA (form 4), not an error"""
    n, d, frac = ref.OVERFLOW
    A, q = ref.fixture(n, d)
    qm = float(np.max(np.abs(q)))
    l1, l2 = np.full(d, 2 * RHO * 0.3 * qm), ref.overflow_l2(d)
    l1[d - 20:] = 0.0
    W, reps = R._lib.k_wstep_ws(A, np.stack([q, q]), RHO, l1=l1, l2=l2, tol=1e-13, ws_cap=16)
    for k in range(2):
        kkt = opref.enet_kkt(A, q, RHO, l1, l2, W[k][:d])
        print(f"free > slots, step {k}: KKT residual {kkt:.3e}, {reps[k]}")
        assert reps[k]["left_route"] == 1 and reps[k]["form"] == 4 and reps[k]["rounds"] == 0
        assert kkt <= KKT * max(1.0, qm) and W[k][d - 1] != 0.0    # (an empty free column keeps its 0: its gradient is 0)
    W, reps = R._lib.k_wstep_ws(A, q, RHO, l1=l1, l2=l2, tol=1e-13)          # 1024 slots hold them
    assert reps[0]["form"] == 5 and reps[0]["slots"] >= 20
    assert opref.enet_kkt(A, q, RHO, l1, l2, W[0][:d]) <= KKT * max(1.0, qm)


def test_sequence_on_one_workspace(R, fx):
    """five right-hand sides q_k = q + 0.01 k D^T b' on one working set: from step 1 on few rows of Gs are formed (none when
    the support did not change), every step is KKT-tight, and the bits are those of a second run and of num_cu = 1"""
    A, q, qm, reg, _ = fx[(3000, 16385)]
    d = A.shape[1]
    b2 = np.random.default_rng(11).standard_normal(A.shape[0])
    Q = np.stack([q + 0.01 * k * (A.T @ b2) for k in range(5)] + [q + 0.04 * (A.T @ b2)])   # the last one twice
    W, reps = R._lib.k_wstep_ws(A, Q, RHO, reg=reg, tol=1e-13)
    for k in range(6):
        kkt = opref.enet_kkt(A, Q[k], RHO, reg, None, W[k][:d])
        print(f"step {k}: KKT residual {kkt:.3e}, {reps[k]}")
        assert kkt <= KKT * max(1.0, qm) and reps[k]["form"] == 5 and _plus_zero(W[k][d:])
        if k:
            assert reps[k]["rows_last"] <= reps[k]["slots"] // 4
            if np.array_equal(W[k] != 0, W[k - 1] != 0):
                assert reps[k]["rows_last"] == 0
            assert reps[k]["rows_total"] == reps[k - 1]["rows_total"] + reps[k]["rows_last"]
    assert reps[5]["rows_last"] == 0 and reps[5]["rounds"] == 1 and reps[5]["pass_pairs"] == 1
    assert np.array_equal(_bits(W[5]), _bits(W[4]))          # started at the solution of the same problem
    for num_cu in (0, 1):
        W2, reps2 = R._lib.k_wstep_ws(A, Q, RHO, reg=reg, tol=1e-13, num_cu=num_cu)
        assert np.array_equal(_bits(W2), _bits(W)) and reps2 == reps, num_cu


def test_kernel_entry_refusals(R):
    A = opref.small_matrix()
    q = np.ones(A.shape[1])
    L = R._lib
    with pytest.raises(ValueError, match="bad argument"):
        L.k_wstep_ws(A, q, RHO)                              # neither reg nor penalties
    with pytest.raises(ValueError, match="penalties must be finite and >= 0"):
        L.k_wstep_ws(A, q, RHO, l1=-np.ones(A.shape[1]))
    with pytest.raises(ValueError, match="bad argument"):
        L.k_wstep_ws(A, q, RHO, reg=0.1, ws_cap=L.WS_CAP + 1)
    with pytest.raises(ValueError, match="bad argument"):
        L.k_wset_scan(np.zeros(7), np.zeros(7), np.zeros(7, dtype=np.int32))   # ld odd


# ---------------------------------------------------------------------------------------------------- solver level
@pytest.fixture(scope="module")
def wide():
    """3000 x 20 000, six entries per row, and D = -y [X | 1] (tests/test_gpu_wstep_op.py's)"""
    n = 3000
    X = opref.wide_matrix(n, 20000, per_row=6, seed=77)
    y = np.where(np.random.default_rng(78).standard_normal(n) > 0, 1.0, -1.0)
    D = sp.csr_matrix(sp.hstack([X, np.ones((n, 1))]).multiply(-y[:, None]))
    return X, y, D


def _steps(m, nit):
    stats = [m._s.step(False) for _ in range(nit)]
    return stats, m._s.get_state()


WIDE_CASES = {
    "lasso": dict(weight_function="erm", loss="binary_cross_entropy", l1w=1e-3, l2w=None),
    "elastic_net": dict(weight_function="aorr", loss="hinge", args=[0.2, 0.8], l1w=(1e-5, 3e-5), l2w=(0.005, 0.02)),
}


@pytest.mark.parametrize("case", sorted(WIDE_CASES))
def test_wide_solve_against_the_reference_admm(R, wide, case):
    """d = 20 001 with an unpenalised intercept, 10 iterations: the objective against wstep_op_ref.admm to 2.5e-7 relative,
    every w-step on the working set; the iterate differences to the reference and to l1_solver="fista" are printed.
    The elastic-net case has the penalties of tests/test_gpu_wstep_op.py's: with weaker ones this AoRR trajectory (not a
    convex problem) separates by 6e-7 in the objective between two exact CPU w-steps already - no bar for any solver."""
    X, y, D = wide
    d = D.shape[1]
    c = dict(WIDE_CASES[case])
    l1w, l2w = c.pop("l1w"), c.pop("l2w")
    rng = np.random.default_rng(81)
    l1w = np.full(d - 1, l1w) if np.isscalar(l1w) else rng.uniform(*l1w, d - 1)
    l2w = None if l2w is None else rng.uniform(*l2w, d - 1)
    pen = R._solver.resolve_penalty(d - 1, None, None, l1w, l2w, True)
    want = opref.admm(D, c["weight_function"], c["loss"], pen["l1"], pen["l2"], pen["reg"], args=c.get("args"), iters=10)
    kw = dict(l1_weights=l1w, l2_weights=l2w, fit_intercept=True, storage=ST, max_iter=10, tol=0.0, **c)
    m = R.ADMMmethod(X, y, l1_solver="working_set", **kw)
    m0 = R.ADMMmethod(X, y, **kw)
    try:
        assert m.gram == "none" and m.l1_solver == "working_set" and m0.l1_solver == "fista"
        stats, got = _steps(m, 10)
        stats0, got0 = _steps(m0, 10)
        info = m.wset_info_
        f = m._s.objective(got["w"])
        print(f"{case}: objective {f!r}, reference {want['objective']!r}, fista {m0._s.objective(got0['w'])!r}; "
              f"max |w - ref| {np.max(np.abs(got['w'] - want['w'])):.3e}, max |w - w_fista| {np.max(np.abs(got['w'] - got0['w'])):.3e}; "
              f"inner {[st.inner_iters for st in stats]}, fista inner {[st.inner_iters for st in stats0]}, working set {info}")
        assert all(st.wstep_form == 5 for st in stats), [st.wstep_form for st in stats]
        assert all(st.wstep_form == 4 for st in stats0)
        assert m.gram_info_["route"] == 0
        assert abs(f - want["objective"]) <= OBJ * max(1.0, abs(want["objective"]))
        assert info["form"] == 5 and info["left_route"] == 0 and 0 < info["support"] <= info["slots"] <= R._lib.WS_CAP
        assert info["bytes"] >= 8 * R._lib.WS_CAP ** 2
        with pytest.raises(R._lib.RblError, match="no working set"):
            m0.wset_info_
    finally:
        m._s.close()
        m0._s.close()


def _sparse_problem(n, d, density=0.15):
    from oracle import problems
    X, y = problems.make_problem(n, d, seed=900 + n + d)
    X = X * (np.random.default_rng(n + d).random(X.shape) < density)
    return sp.csr_matrix(X), y


def _run(R, A, y, nit, **pr):
    m = R.ADMMmethod(A, y, max_iter=nit, tol=0.0, storage=ST, gram="none", **pr)
    forms = [m._s.step(False).wstep_form for _ in range(nit)]
    return m, m._s.get_state(), forms


@contextlib.contextmanager
def _second_handle(R):
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
    A, y = _sparse_problem(400, 61)
    nit = 8
    members = [dict(weight_function="superquantile", loss="binary_cross_entropy", l1_reg=r, args=[a])
               for a, r in ((0.5, 0.01), (0.9, 0.02), (0.3, 0.005))]
    g = R.ADMMgroup(A, y, [dict(pr, gram="none", share_sparse=share, l1_solver="working_set") for pr in members], storage=ST,
                    max_iter=nit, tol=0.0)
    try:
        _quiet(g.main_loop, False)
        assert all(st.wstep_form == 5 for st in g.last)
        assert (g.counters()["shared_v"] > 0) == share
        states = [s._s.get_state() for s in g.solvers]
        assert all(s.wset_info_["form"] == 5 for s in g.solvers)          # a working set each
    finally:
        g.close()
    for k, pr in enumerate(members):
        with _second_handle(R):
            m, own, forms = _run(R, A, y, nit, l1_solver="working_set", **pr)
            m._s.close()
        assert all(f == 5 for f in forms)
        _same_state(states[k], own, (share, k))


@pytest.mark.parametrize("share", [False, True])
def test_one_vs_rest_members_equal_their_standalone_solves(R, share):
    A, _ = _sparse_problem(400, 61)
    labels = np.arange(400) % 3
    nit = 8
    ovr = R.OneVsRest(A, labels, l1_reg=0.01, storage=ST, max_iter=nit, tol=0.0, gram="none", share_sparse=share,
                      l1_solver="working_set")
    try:
        _quiet(ovr.main_loop, False)
        assert all(st.wstep_form == 5 for st in ovr.group.last)
        states = [s._s.get_state() for s in ovr.group.solvers]
    finally:
        ovr.close()
    for k, c in enumerate(ovr.classes_):
        with _second_handle(R):
            m, own, forms = _run(R, A, np.where(labels == c, 1.0, -1.0), nit, weight_function="erm",
                                 loss="binary_cross_entropy", l1_reg=0.01, l1_solver="working_set")
            m._s.close()
        _same_state(states[k], own, (share, k))


def test_second_upload_drops_the_sub_gram_matrix(R):
    """other entries uploaded on the same handle: the next solve equals a fresh handle's bit for bit"""
    A, y = _sparse_problem(400, 61)
    B, yb = _sparse_problem(400, 61, density=0.2)
    B = sp.csr_matrix(B.multiply(1.5))
    pr = dict(weight_function="erm", loss="binary_cross_entropy", l1_reg=0.01, l1_solver="working_set")
    m, _, forms = _run(R, A, y, 6, **pr)
    fresh = R.ADMMmethod(B, yb, max_iter=6, tol=0.0, storage=ST, gram="none", **pr)
    try:
        assert all(f == 5 for f in forms) and m.wset_info_["rows_total"] > 0
        z0 = fresh._s.get_state()                                        # the state every handle starts from
        assert all(fresh._s.step(False).wstep_form == 5 for _ in range(6))
        want = fresh._s.get_state()
        s = m._s
        s.set_data(B, yb)
        s.gram()
        s.set_state(w=z0["w"], z=z0["z"], lam=z0["lam"], rho=z0["rho"], iter=0)
        assert all(s.step(False).wstep_form == 5 for _ in range(6))
        _same_state(s.get_state(), want, "second upload")
        assert m.wset_info_["rows_total"] <= m.wset_info_["slots"]      # counted again from the empty set
    finally:
        m._s.close()
        fresh._s.close()


def test_set_state_with_a_support_outside_the_working_set(R):
    A, y = _sparse_problem(400, 61)
    pr = dict(weight_function="erm", loss="binary_cross_entropy", l1_reg=0.004, l1_solver="working_set")
    m, st, forms = _run(R, A, y, 6, **pr)
    try:
        s = m._s
        inside = st["w"] != 0
        print("support before set_state:", int(inside.sum()))
        assert inside.sum() <= 56
        w_new = np.zeros(61)
        outside = np.flatnonzero(~inside)[:5]
        w_new[outside] = 0.3                                             # a support S does not hold
        s.set_state(w=w_new)
        stat = s.step(False)
        info = m.wset_info_
        assert stat.wstep_form == 5 and info["left_route"] == 0
        # the w-step's own problem: q and rho of that step, read back, and the KKT conditions of the w it returned
        q = _dev(*s.buffer(R._lib.BUF_Q))[:61]
        w = s.get_state()["w"]
        D = sp.csr_matrix(A.multiply(-np.asarray(y).reshape(-1, 1)))
        kkt = opref.enet_kkt(D, q, stat.rho, 0.004, None, w)
        print(f"set_state: KKT residual {kkt:.3e}, working set {info}")
        assert kkt <= KKT * max(1.0, float(np.max(np.abs(q))))
        assert info["support"] == np.count_nonzero(w)
    finally:
        m._s.close()


def test_redone_w_step_finds_the_restored_support_again(R, monkeypatch):
    """The banded z-step of a superquantile handle is given an m it cannot certify (all rows equal: zband == 2), so
    rbl_phase_w restores w from w_prev and runs the w-step a second time.  w_prev is dense over 1500 columns - wider than
    the working set - so the first pass had cold-started S from w = 0: the second pass must find the restored support
    again (here: cold-start again), not keep 1500 stale coefficients outside S.  X holds small integers and w_prev is
    2^-10 everywhere, so D w_prev is exact in any order and m = D w_prev - lambda / rho is 0.75 in every row, in bits."""
    import zstep_inject as Z
    for k, v in {"RBL_NO_ZBAND": "0", "RBL_NO_SORT32": "0", "RBL_ZBAND_MIN_N": "16"}.items():
        monkeypatch.setenv(k, v)
    n, d, rho, reg = 4096, 1500, 2.0 ** -4, 0.05
    rng = np.random.default_rng(12)
    X = sp.random(n, d, density=0.02, random_state=np.random.RandomState(12), format="csr",
                  data_rvs=lambda k: rng.choice([-2.0, -1.0, 1.0, 2.0], k))
    y = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    D = sp.csr_matrix(X.multiply(-y[:, None]))
    w0 = np.full(d, 2.0 ** -10)
    m = Z.pattern("all_equal", n, 1, "superq_0.5")
    lam = rho * (D @ w0 - m)
    assert np.array_equal(D @ w0 - lam / rho, m)
    s = R.Solver(n, d, "superquantile", Z.BCE, reg=reg, wstep=R._lib.WSTEP_L1, args=[0.5], tol=0.0, storage=ST, gram="none",
                 l1_solver="working_set")
    try:
        s.set_data(X, y)
        s.gram()
        s.set_state(w=w0, lam=lam, rho=rho, iter=200)
        st = s.step(False)
        info = s.wset_info()
        w = s.get_state(want_z=False, want_lam=False)["w"]
        q = _dev(*s.buffer(R._lib.BUF_Q))[:d]
        kkt = opref.enet_kkt(D, q, st.rho, reg, None, w)
        print(f"redone w-step: zband {st.zband}, form {st.wstep_form}, support {np.count_nonzero(w)}, KKT residual {kkt:.3e}, {info}")
        assert st.zband == 2                                 # the z-step was not certified: z, q and the w-step were redone
        assert st.wstep_form == 5 and info["left_route"] == 0
        assert 0 < np.count_nonzero(w) == info["support"] <= info["slots"] < d
        assert kkt <= KKT * max(1.0, float(np.max(np.abs(q))))
    finally:
        s.close()


def test_default_and_fista_reproduce_the_parent_commit(R):
    """erm / BCE / l1 on 400 x 61 with gram="none", 8 iterations: w, z, lambda of the parent commit's library (written on an
    MI355X before this route existed) - bit for bit, by default and with l1_solver="fista" spelled out"""
    gold = np.load(GOLDEN)
    A, y = _sparse_problem(400, 61)
    for kw in ({}, dict(l1_solver="fista")):
        m, st, forms = _run(R, A, y, 8, weight_function="erm", loss="binary_cross_entropy", l1_reg=0.01, **kw)
        m._s.close()
        assert all(f == 4 for f in forms)
        for key in ("w", "z", "lam"):
            assert np.array_equal(_bits(st[key]), _bits(gold[key])), (kw, key)
        assert st["rho"] == float(gold["rho"])


def _cfg(L, n, d, storage, wstep=1, objective_only=0):
    cfg = L.RblConfig()
    cfg.n, cfg.d, cfg.n_total, cfg.row_offset = n, d, n, 0
    cfg.loss, cfg.weight_function = L.LOSS["binary_cross_entropy"], L.WEIGHT["erm"]
    cfg.wstep, cfg.reg, cfg.smooth_t, cfg.tol, cfg.max_iter = wstep, 0.01, 1.0, 1e-4, 10
    cfg.storage, cfg.device, cfg.objective_only = L.STORAGE[storage], 0, objective_only
    return cfg


def test_create_time_refusals_of_the_flag(R):
    L = R._lib
    lib = L.load()
    h = C.c_void_p()
    WS, NG = L.CREATE_WORKING_SET, L.CREATE_NO_GRAM
    assert lib.rbl_create_opts(C.byref(_cfg(L, 50, 20, "csr")), WS, C.byref(h)) == L.RBL_ERR_INVALID and not h.value
    assert "RBL_CREATE_WORKING_SET needs RBL_CREATE_NO_GRAM" in L.last_error()
    assert lib.rbl_create_opts(C.byref(_cfg(L, 50, 20, "csr", wstep=L.WSTEP_L2)), WS | NG, C.byref(h)) == L.RBL_ERR_INVALID
    assert "needs cfg.wstep == RBL_WSTEP_L1" in L.last_error() and not h.value
    assert lib.rbl_create_opts(C.byref(_cfg(L, 50, 20, "f64")), WS | NG, C.byref(h)) == L.RBL_ERR_INVALID
    assert "needs RBL_STORE_CSR" in L.last_error()
    assert lib.rbl_create_opts(C.byref(_cfg(L, 50, 20, "csr")), 4, C.byref(h)) == L.RBL_ERR_INVALID
    assert "unknown flag bits 0x4" in L.last_error()
    assert lib.rbl_create_opts(C.byref(_cfg(L, 50, 20, "csr")), WS | NG, C.byref(h)) == L.RBL_OK
    rep = L.RblWsetReport()
    assert lib.rbl_wset_info(h, C.byref(rep)) == L.RBL_OK and rep.form == 0 and rep.slots == 0 and rep.bytes >= 8 * L.WS_CAP ** 2
    assert lib.rbl_wset_info(h, None) == L.RBL_ERR_INVALID
    lib.rbl_destroy(h)
    # a borrower of such an owner: a working set of its own under the same rule
    A, y = _sparse_problem(400, 61)
    m = R.ADMMmethod(A, y, l1_reg=0.01, storage=ST, gram="none", l1_solver="working_set")
    try:
        assert lib.rbl_create_shared(C.byref(_cfg(L, 400, 61, "csr", wstep=L.WSTEP_L2)), m._s._h, C.byref(h)) == L.RBL_ERR_INVALID
        assert "needs cfg.wstep == RBL_WSTEP_L1" in L.last_error() and not h.value
        assert lib.rbl_create_shared(C.byref(_cfg(L, 400, 61, "csr")), m._s._h, C.byref(h)) == L.RBL_OK
        st = L.RblStats()
        assert lib.rbl_step(h, 0, C.byref(st)) == L.RBL_OK and st.wstep_form == 5
        assert lib.rbl_wset_info(h, C.byref(rep)) == L.RBL_OK and rep.form == 5
        lib.rbl_destroy(h)
        with pytest.raises(ValueError, match="a borrower follows its owner"):
            R.ADMMmethod(A, y, l1_reg=0.02, storage=ST, gram="none", share_data=m)
    finally:
        m._s.close()
