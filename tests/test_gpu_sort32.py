"""The z-step's sort with 32-bit keys (csrc/elementwise.hip: k_make_m_range, k_keys32, k_sort32_fix; csrc/api_iter.hip:
z_step_sorted, zb_resolve) driven on purpose.

Kernel level (rbl_k_sort32 runs exactly the launches of the z-step's 32-bit branch): the permutation and the sorted m,
bit for bit, against NumPy's stable argsort, on inputs whose runs of equal keys are designed - exact duplicates up to
the limit of 32 and one past it, near ties the stable sort delivers in the wrong order, runs across the fix-up's blocks
and the sort's tiles, the saturated key, degenerate and overflowing ranges, row offsets, signed zeros.  With the flag
raised only the flag is asserted: the values are documented as meaningless.

Solver level: a designed m through the state of a handle, the redo with 64-bit keys after rbl_phase_q, the pause of 64
iterations and the return to 32-bit keys, bit identity with a run under RBL_NO_SORT32=1, a read of z in mid-iteration,
and a group.

Every statement about an input (longest run, expected flag) comes from oracle/sort32.py and is pinned on a CPU by
test_sort32_host.py; none is taken from a device run.  NaN in m is not tested: a solve produces one only after it has
diverged."""
import numpy as np
import pytest

import sort32_fixtures as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def R():
    import admm_for_rank_based_loss_amd as rbl
    if rbl._lib.device_count() < 1:
        pytest.fail("no HIP device: the GPU tests must run the HIP library (no fallback)")
    return rbl


@pytest.fixture(scope="module")
def L(R):
    return R._lib


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check(L, m, idx_off, flag_ref, ms_ref, ids0_ref):
    ms, ids, flag = L.k_sort32(m, idx_off)
    assert flag == flag_ref
    if flag_ref:
        return None
    ids_ref = (ids0_ref.astype(np.uint64) + np.uint64(idx_off)).astype(np.uint32)
    assert np.array_equal(ids, ids_ref)
    assert np.array_equal(_bits(ms), _bits(ms_ref))
    return ms, ids


# ------------------------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("name", F.NAMES)
def test_sort32_bit_exact(L, name):
    """(m, row) order bit for bit; the flag exactly where the restatement finds a run of more than 32; on flag-0 inputs
    without signed zeros the 64-bit sort's output, bit for bit; a second call gives the same bits"""
    m = F.get(name)
    run, flag_ref, order, ms_ref, ids_ref = F.reference(name)
    out = _check(L, m, 0, flag_ref, ms_ref, ids_ref)
    again = L.k_sort32(m, 0)
    assert again[2] == flag_ref
    if out is None:
        return
    assert np.array_equal(again[1], out[1]) and np.array_equal(_bits(again[0]), _bits(out[0]))
    if not F.has_signed_zeros(name):
        k64, p64 = L.k_sort(m)
        assert np.array_equal(p64, out[1]) and np.array_equal(_bits(k64), _bits(out[0]))


def test_sort32_all_equal_is_the_identity(L):
    ms, ids, flag = L.k_sort32(F.get("all_equal_32"))
    assert flag == 0 and np.array_equal(ids, np.arange(32, dtype=np.uint32))


@pytest.mark.parametrize("name", ["gauss_4097", "dup_x32", "run32_after_4095", "near_ties", "dup_x33"])
def test_sort32_row_offset(L, name):
    """the row ids carry the offset of a shard (the fix-up reads m at id - offset, in 32-bit arithmetic)"""
    m = F.get(name)
    run, flag_ref, order, ms_ref, ids_ref = F.reference(name)
    for off in (1000, (1 << 32) - m.size):
        _check(L, m, off, flag_ref, ms_ref, ids_ref)
    with pytest.raises(ValueError):
        L.k_sort32(m, (1 << 32) - m.size + 1)


def test_sort32_signed_zeros_keep_row_order(L):
    """the 32-bit path compares m numerically: -0.0 and +0.0 tie and keep their row order, as NumPy's stable argsort
    (and the reference's) does; the 64-bit sort orders the bit patterns (test_sort_bit_exact pins that one)"""
    m = F.get("signed_zeros")                          # [0.0, -0.0, 1.0, -1.0, -0.0, 0.0, -0.0]
    ms, ids, flag = L.k_sort32(m)
    assert flag == 0 and list(ids) == [3, 0, 1, 4, 5, 6, 2]
    assert np.array_equal(_bits(ms), _bits(m[[3, 0, 1, 4, 5, 6, 2]]))
    k64, p64 = L.k_sort(m)
    assert list(p64) == [3, 1, 4, 6, 0, 5, 2]


# ------------------------------------------------------------------------------------------------ solver level
_WSTEP = {"l1": 1, "l2": 2}


def _solver(R, X, y, weight_function, loss, reg, wstep, args=None, B=None):
    s = R.Solver(X.shape[0], X.shape[1], weight_function, loss, reg=reg, wstep=_WSTEP[wstep], args=args, B=B, tol=0.0,
                 storage="f64")
    s.set_data(X, y)
    return s


DESIGNED = [
    ("extremile_bce", "extremile", "binary_cross_entropy", [2.0], None),
    ("esrm_bce", "esrm", "binary_cross_entropy", [1.0], None),
    ("ehrm_bce", "ehrm", "binary_cross_entropy", None, -5.0),
    ("esrm_hinge", "esrm", "hinge", [1.0], None),
]


def _z_of_designed_m(R, wf, loss, args, B, m_target):
    """one z-step of a handle whose state makes m = 0 - (-m_target) / 1 = m_target exactly; returns (z read before
    the w-step - the read settles the verdict -, sort_passes of the iteration)"""
    from oracle import problems
    n = m_target.size
    X, y = problems.make_problem(n, 8, seed=4)
    s = _solver(R, X, y, wf, loss, 0.01, "l2", args, B)
    s.set_state(w=np.zeros(8), lam=-m_target, rho=1.0, iter=3)
    s.phase_m()
    s.phase_z()
    z = s.get_state(want_lam=False)["z"].copy()
    s.phase_q()
    s.phase_w()
    s.phase_dual()
    st = s.phase_finish()
    s.close()
    return z, st.sort_passes


@pytest.mark.parametrize("fixture", ["run32_after_4080", "run33_after_4080"])
@pytest.mark.parametrize("name,wf,loss,args,B", DESIGNED, ids=[c[0] for c in DESIGNED])
def test_designed_m_through_the_state(R, name, wf, loss, args, B, fixture):
    """a run of 32 is repaired by the fix-up (4 radix passes), a run of 33 is flagged and the step redone with 64-bit
    keys (4 + 8); z against the oracle's exact z-step either way, to the bound test_pav_many_sizes_vs_oracle uses for
    the same PAV"""
    from oracle import admm, weights
    m_target = np.array(F.get(fixture))
    flag_ref = F.reference(fixture)[1]
    z, passes = _z_of_designed_m(R, wf, loss, args, B, m_target)
    sa, sb = weights.get_weights(wf, m_target.size, args)
    zref, _ = admm.z_step_exact(wf, loss, sa, sb, B, 1.0, m_target)
    err = np.max(np.abs(z - zref))
    print(f"{name} {fixture}: max|z - z_oracle| = {err:.3e}, sort_passes = {passes}")
    assert passes == (12 if flag_ref else 4)
    assert err <= 1e-9 * max(1.0, np.max(np.abs(zref)))


@pytest.mark.parametrize("loss", ["binary_cross_entropy", "hinge"])
def test_designed_m_ties_across_the_band_edges(R, loss, monkeypatch):
    """aorr [0.2, 0.8] through the sort (RBL_NO_ZBAND=1): eight exactly equal m across each rank where the weights
    change - the row order inside the run decides which rows get zero weight, so a wrong permutation moves z by
    O(sigma / rho)"""
    from oracle import admm, weights
    monkeypatch.setenv("RBL_NO_ZBAND", "1")
    m_target = np.array(F.get("band_edge_runs"))
    assert F.reference("band_edge_runs")[1] == 0
    z, passes = _z_of_designed_m(R, "aorr", loss, [0.2, 0.8], None, m_target)
    sa, sb = weights.get_weights("aorr", m_target.size, [0.2, 0.8])
    zref, _ = admm.z_step_exact("aorr", loss, sa, sb, None, 1.0, m_target)
    err = np.max(np.abs(z - zref))
    print(f"aorr {loss}: max|z - z_oracle| = {err:.3e}, sort_passes = {passes}")
    assert passes == 4
    assert err <= 1e-9 * max(1.0, np.max(np.abs(zref)))


def _kw_solver(R, X, y, kw):
    l1 = "l1_reg" in kw
    return _solver(R, X, y, kw["weight_function"], kw["loss"], kw["l1_reg"] if l1 else kw["l2_reg"], "l1" if l1 else "l2",
                   kw.get("args"), kw.get("B"))


@pytest.mark.parametrize("case", list(F.REPLICATED_CASES))
def test_redo_pause_and_return(R, case):
    """every row 33 times: each attempt with 32-bit keys is flagged.  Iteration 0 sorts 64-bit keys (8 passes),
    iteration 1 tries 32-bit keys and is redone (4 + 8) - after rbl_phase_q, so q is redone as well and the w-step
    runs again from w_k -, the next 64 iterations stay on 64-bit keys, iteration 66 tries again.  Iterates against the
    oracle's exact mode with the bars of test_iterates_match_oracle_exact."""
    from oracle import admm
    kw = F.REPLICATED_CASES[case]
    X, y = F.replicated_problem(33)
    nit = 70
    ref = admm.admm_solve(X, y, max_iter=nit, mode="exact", tol=0.0, **kw)
    s = _kw_solver(R, X, y, kw)
    tol = 1e-9 if kw["loss"] == "binary_cross_entropy" else 1e-7
    passes = []
    for i in range(nit):
        st = s.step(True)
        passes.append(st.sort_passes)
        assert abs(st.rho - ref.rho[i]) <= 1e-15 * ref.rho[i]
        assert abs(st.primal - ref.primal[i]) <= tol * max(1.0, ref.primal[i]), (i, st.primal, ref.primal[i], passes)
        assert abs(st.dual - ref.dual[i]) <= tol * max(1.0, ref.dual[i]), (i, passes)
        assert abs(st.objective - ref.objective[i + 1]) <= tol * max(1.0, abs(ref.objective[i + 1])), (i, passes)
    assert passes == [8, 12] + [8] * 64 + [12] + [8] * 3, passes
    state = s.get_state()
    assert np.max(np.abs(state["w"] - ref.w)) <= tol * max(1.0, np.max(np.abs(ref.w)))
    assert np.max(np.abs(state["z"] - ref.z)) <= 10 * tol * max(1.0, np.max(np.abs(ref.z)))
    assert np.max(np.abs(state["lam"] - ref.lam)) <= 10 * tol * max(1e-3, np.max(np.abs(ref.lam)))
    s.close()


@pytest.mark.parametrize("case", list(F.REPLICATED_CASES))
def test_runs_of_32_are_repaired_in_every_iteration(R, case):
    """every row 32 times: the restatement finds a longest run of exactly 32 in iterations 1 ... 11 of the oracle's
    trajectory, with the tied groups thousands of key spacings apart (test_sort32_host.py) - 4 passes, never a redo"""
    from oracle import admm
    kw = F.REPLICATED_CASES[case]
    X, y = F.replicated_problem(32)
    nit = 12
    ref = admm.admm_solve(X, y, max_iter=nit, mode="exact", tol=0.0, **kw)
    s = _kw_solver(R, X, y, kw)
    passes = [s.step(False).sort_passes for _ in range(nit)]
    assert passes == [8] + [4] * (nit - 1), passes
    tol = 1e-9 if kw["loss"] == "binary_cross_entropy" else 1e-7
    state = s.get_state()
    assert np.max(np.abs(state["w"] - ref.w)) <= tol * max(1.0, np.max(np.abs(ref.w)))
    assert np.max(np.abs(state["z"] - ref.z)) <= 10 * tol * max(1.0, np.max(np.abs(ref.z)))
    s.close()


IDENTITY = list(F.IDENTITY_CASES.items())


def _follows_the_32bit_schedule(passes):
    """iteration 0: 8; then 4 (certified) or 12 (redone), and 8 during the 64 iterations after a redo"""
    skip_until, seen = 0, set()
    for k, p in enumerate(passes):
        if k == 0 or k < skip_until:
            if p != 8:
                return False, seen
        else:
            if p not in (4, 12):
                return False, seen
            seen.add(p)
            if p == 12:
                skip_until = k + 1 + 64
    return True, seen


@pytest.mark.parametrize("data", ["gaussian", "rows_x33"])
@pytest.mark.parametrize("name,kw", IDENTITY, ids=[c[0] for c in IDENTITY])
def test_32bit_and_64bit_keys_give_the_same_bits(R, name, kw, data, monkeypatch):
    """a default run against a run under RBL_NO_SORT32=1: the sorted m and the permutation are the same bits on both
    paths, so w, z, lambda and the residuals must be, after every iteration"""
    X, y = F.gaussian_problem() if data == "gaussian" else F.replicated_problem(33)
    nit = 14

    def run(no32):
        monkeypatch.setenv("RBL_NO_SORT32", "1" if no32 else "0")
        s = _kw_solver(R, X, y, kw)
        out = []
        for _ in range(nit):
            st = s.step(False)
            state = s.get_state()
            out.append((st.sort_passes, st.primal, st.dual, state["w"].copy(), state["z"].copy(), state["lam"].copy()))
        s.close()
        return out

    a, b = run(False), run(True)
    pa, pb = [o[0] for o in a], [o[0] for o in b]
    ok, seen = _follows_the_32bit_schedule(pa)
    assert ok and seen, pa
    if data == "gaussian":
        assert pa == [8] + [4] * (nit - 1), pa                # runs of 1 - 3 keys in every iteration (test_sort32_host.py)
    else:
        assert pa[1] == 12, pa                                # a run of 33 at iteration 1
    assert pb == [8] * nit, pb
    for k in range(nit):
        assert a[k][1:3] == b[k][1:3], (k, pa)
        for j in (3, 4, 5):
            assert np.array_equal(a[k][j], b[k][j]), (k, j, pa, np.max(np.abs(a[k][j] - b[k][j])))


def test_reading_z_mid_iteration_settles_the_32bit_sort(R):
    """an overridden w_subproblem that reads z before the library's w-step, on the 33-fold rows: the read settles the
    verdict (the z it gets is the redone one), and the trajectory is that of the run that never looks, bit for bit"""
    from admm_for_rank_based_loss_amd.src.optim.algorithms import Optimizer
    X, y = F.replicated_problem(33)
    kw = dict(F.REPLICATED_CASES["extremile_bce_l1"], max_iter=14, tol=0.0, storage="f64")

    class Peek(R.ADMMmethod):
        peeked = None

        def w_subproblem(self):
            self.peeked.append(self._s.get_state(want_lam=False)["z"].copy())
            return super().w_subproblem()

    runs = []
    for cls in (R.ADMMmethod, Peek):
        s = cls(X, y, **kw)
        s.peeked = []
        passes, zs = [], []
        for i in range(kw["max_iter"]):
            Optimizer.main_loop(s, i, 0.0, False)
            passes.append(s._last.sort_passes)
            zs.append(s._s.get_state(want_lam=False)["z"].copy())
        runs.append((s._s.get_state(), passes, s.peeked, zs))
    (a, pa, _, _), (b, pb, peeked, zs) = runs
    assert pa == pb == [8, 12] + [8] * 12, (pa, pb)
    assert np.array_equal(a["w"], b["w"]) and np.array_equal(a["z"], b["z"]) and np.array_equal(a["lam"], b["lam"])
    assert len(peeked) == len(zs)
    for k in range(len(zs)):
        assert np.array_equal(peeked[k], zs[k]), k          # what the hook saw is that iteration's final z


def test_group_members_redo_inside_the_group_step(R):
    """extremile and ESRM members on 33-fold rows (d = 160: from 65 columns on a group shares its passes over D): the
    redo with 64-bit keys happens inside rbl_group_step, each member's iterates equal its standalone handle bit for
    bit, and the pass counters follow the accounting of test_gpu_group.py - a member's own n x d launches are its
    first v = D w plus one q per redone z-step"""
    X, y = F.replicated_problem(33, n0=200, d=160)
    members = [
        dict(weight_function="extremile", loss="binary_cross_entropy", l1_reg=0.01, args=[2.0]),
        dict(weight_function="esrm", loss="hinge", l2_reg=0.01, args=[1.0]),
        dict(weight_function="extremile", loss="binary_cross_entropy", l2_reg=0.01, args=[3.0]),
        dict(weight_function="esrm", loss="binary_cross_entropy", l2_reg=0.01, args=[2.0]),
    ]
    K, nit = len(members), 6
    solvers = []
    for pr in members:
        solvers.append(R.ADMMmethod(X, y, max_iter=nit, tol=0.0, storage="f64",
                                    share_data=solvers[0] if solvers else None, **pr))
    g = R._solver.Group([s._s for s in solvers])
    redone, single, passes = np.zeros((nit, K), dtype=int), [], []
    for i in range(nit):
        stats = g.step(want_objective=False)
        passes.append([st.sort_passes for st in stats])
        redone[i] = [int(st.zband == 2) + int(st.sort_passes == 12) for st in stats]
        single.append(np.array(g.counters()["single_passes"]))
    cnt = g.counters()
    single = np.array(single)
    assert passes == [[8] * K, [12] * K] + [[8] * K] * (nit - 2), passes
    kpp = cnt["k_per_pass"]
    assert kpp >= 2
    assert cnt["shared_v"] == cnt["shared_q"] == nit * -(-K // kpp), cnt
    assert list(single[0]) == [1 + r for r in redone[0]], (single[0], redone[0])
    assert np.array_equal(single[-1] - single[0], redone[1:].sum(axis=0)), (single, redone)
    states = [s._s.get_state() for s in solvers]
    for k, pr in enumerate(members):
        alone = R.ADMMmethod(X, y, max_iter=nit, tol=0.0, storage="f64", **pr)
        pk = [alone._s.step(False).sort_passes for _ in range(nit)]
        assert pk == [p[k] for p in passes], (k, pk)
        st = alone._s.get_state()
        for key in ("w", "z", "lam"):
            assert np.array_equal(states[k][key], st[key]), (k, key)
        alone._s.close()
    g.close()
